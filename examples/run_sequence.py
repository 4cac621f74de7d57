"""Run LiDAR SLAM on a folder of scans.

    python examples/run_sequence.py <folder> [--gt poses_tum.txt] [--gt-mesh mesh.ply [--mesh-resolution 0.1] [--tsdf-baseline [--tsdf-sparse]]]
                                    [--out ~/LonerSLAM/outputs] [--name run] [--ray-range 1 50]
                                    [--icp-estimation GENERALIZED] [--icp-kernel tukey 3] [--pose-graph]

<folder> holds one `.npy` file per scan, [N,4] columns x, y, z, t (t: per-point time, local to the scan or global, seconds or
nanoseconds), read in sorted name order, and `stamps.txt` with one scan time in seconds per line.  With --gt (a TUM file: ts x y z qx
qy qz qw) every scan gets the ground-truth pose nearest in time, the world cube is computed from the ground truth and the estimated
trajectory is scored against it; without it the cube comes from system.world_cube.trajectory_bounding_box.  With --gt-mesh (the
.ply the scans were simulated from, or surveyed) the trained map is meshed at --mesh-resolution over the ground-truth mesh's box grown
by 1 m, written to <log>/meshes/, and scored against that mesh with the exact point-to-surface distance
(mesh_eval.evaluate_mesh_to_mesh).  With --tsdf-baseline (needs --gt-mesh) the scan files are then read again and fused into a TSDF
volume (analysis/tsdf.py) along estimated_trajectory.txt and, with --gt, along the ground truth, every ray from the pose at its own
time; both volumes are meshed at --mesh-resolution over the same box, written beside the neural mesh and scored the same way: the
ground-truth one shows what the scans support at that resolution, the estimated one what the tracking costs.  With --tsdf-sparse
(only with --tsdf-baseline) the volumes are SparseTSDFVolumes over the same box: the same meshes and scores from the blocks the rays
wrote to instead of the whole lattice.  The log directory holds the checkpoints, the four trajectory files and the configuration, as the
analysis tools of this package expect them.  With --pose-graph the scans are read again after the run, registered pairwise along
estimated_trajectory.txt (consecutive scans, and scans whose estimated positions lie within --loop-radius and at least --loop-gap
frames apart: no place recognition) and the pose graph is optimised (analysis/pose_graph.py); the result goes to
trajectory/pose_graph_trajectory.txt beside the four files, and with --gt its APE is printed after the run's."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loner_amd.analysis.trajectory import ape, associate                     # noqa: E402
from loner_amd.common.pose import Pose                                       # noqa: E402
from loner_amd.common.pose_utils import build_poses_from_df, read_tum        # noqa: E402
from loner_amd.common.sensors import build_scan_from_points                  # noqa: E402
from loner_amd.common.settings import default_settings                       # noqa: E402
from loner_amd.loner import Loner                                            # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("folder")
    ap.add_argument("--gt")
    ap.add_argument("--gt-mesh")
    ap.add_argument("--mesh-resolution", type=float, default=0.1)
    ap.add_argument("--tsdf-baseline", action="store_true")
    ap.add_argument("--tsdf-sparse", action="store_true", help="with --tsdf-baseline: fuse into a block-sparse volume")
    ap.add_argument("--out", default="~/LonerSLAM/outputs")
    ap.add_argument("--name", default=None)
    ap.add_argument("--ray-range", type=float, nargs=2, default=(1.0, 50.0))
    ap.add_argument("--log-level", default="STANDARD", choices=("DISABLED", "STANDARD", "VERBOSE"))
    ap.add_argument("--icp-estimation", default="POINT_TO_PLANE", choices=("POINT_TO_PLANE", "GENERALIZED"),
                    help="the tracker's estimator (tracker.icp.estimation)")
    ap.add_argument("--icp-kernel", nargs=2, metavar=("TYPE", "K"), default=None,
                    help="a robust loss on the tracker's ICP: huber, cauchy or tukey and its scale (tracker.icp.robust_kernel)")
    ap.add_argument("--pose-graph", action="store_true", help="refine estimated_trajectory.txt by multiway registration")
    ap.add_argument("--loop-radius", type=float, default=3.0, help="with --pose-graph: loop candidates lie within this distance (m)")
    ap.add_argument("--loop-gap", type=int, default=4, help="with --pose-graph: and at least this many frames apart")
    ap.add_argument("--pose-graph-distance", type=float, default=0.5, help="with --pose-graph: the correspondence distance (m)")
    args = ap.parse_args()
    if args.tsdf_baseline and not args.gt_mesh:
        raise SystemExit("--tsdf-baseline needs --gt-mesh")

    files = sorted(glob.glob(os.path.join(args.folder, "*.npy")))
    stamps = np.loadtxt(os.path.join(args.folder, "stamps.txt"), dtype=np.float64, ndmin=1)
    if len(files) == 0 or len(files) != len(stamps):
        raise SystemExit(f"{args.folder}: {len(files)} scans and {len(stamps)} stamps")

    settings = default_settings(args.out, args.ray_range)
    settings["system"]["single_threaded"] = True
    settings["mapper"]["log_level"] = args.log_level
    settings["tracker"]["icp"]["estimation"] = args.icp_estimation
    if args.icp_kernel:
        settings["tracker"]["icp"]["robust_kernel"] = {"type": args.icp_kernel[0], "k": float(args.icp_kernel[1])}
    gt_poses, gt_of_scan = None, None
    if args.gt:
        rows = read_tum(args.gt)
        gt_poses, _ = build_poses_from_df(rows, zero_origin=False)
        scan_idx, gt_idx = associate(stamps, rows[:, 0], t_max_diff=np.inf)
        gt_of_scan = dict(zip(scan_idx.tolist(), gt_idx.tolist()))

    loner = Loner(settings)
    loner.initialize(None, gt_poses, None, list(args.ray_range), None, args.folder, experiment_name=args.name,
                     traj_bounding_box=None if args.gt else settings["system"]["world_cube"]["trajectory_bounding_box"])
    loner.start()
    fov = settings.system.lidar_fov
    for k, (path, stamp) in enumerate(zip(files, stamps)):
        points = np.load(path)
        if points.ndim != 2 or points.shape[1] != 4:
            raise SystemExit(f"{path}: expected [N,4] (x, y, z, t), got {points.shape}")
        scan, _ = build_scan_from_points(points[:, :3].astype(np.float32), points[:, 3], float(stamp), fov=fov)
        gt_pose = Pose(gt_poses[gt_of_scan[k]].clone()) if gt_of_scan is not None and k in gt_of_scan else None
        loner.process_lidar(scan, gt_pose)
    loner.stop()
    log = loner.get_log_directory()
    print(f"log directory: {log}")
    if args.gt:
        score = ape(os.path.join(log, "trajectory", "estimated_trajectory.txt"), args.gt)
        print("APE (aligned, m): " + ", ".join(f"{k} {score[k]:.4f}" for k in ("rmse", "mean", "median", "std", "min", "max")))
    if args.pose_graph:
        pose_graph_refine(files, stamps, fov, loner._mapper._optimizer._device, log, args)
    if args.gt_mesh:
        score_against_mesh(loner, args.gt_mesh, args.mesh_resolution, args.ray_range, log)
    if args.tsdf_baseline:
        device = loner._mapper._optimizer._device
        scans = reread_scans(files, stamps, fov, device)
        tsdf_baseline("estimated trajectory", "estimated", scans, os.path.join(log, "trajectory", "estimated_trajectory.txt"), args.gt_mesh,
                      args.mesh_resolution, log, device, args.tsdf_sparse)
        if args.gt:
            tsdf_baseline("ground-truth trajectory", "gt", scans, args.gt, args.gt_mesh, args.mesh_resolution, log, device, args.tsdf_sparse)


def score_against_mesh(loner, gt_mesh_path, resolution, ray_range, log):
    """Mesh the map the run trained and print evaluate_mesh_to_mesh against the ground-truth mesh"""
    from loner_amd.analysis.mesh_eval import evaluate_mesh_to_mesh
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    gt_mesh = TriangleMesh.read_ply(gt_mesh_path)
    bound = np.stack([gt_mesh.vertices.min(axis=0) - 1.0, gt_mesh.vertices.max(axis=0) + 1.0], axis=1)
    opt = loner._mapper._optimizer
    ckpt = {"poses": loner._mapper._keyframe_manager.get_poses_state()}
    mesher = Mesher(opt._model, ckpt, loner.get_world_cube(), torch.tensor(list(ray_range)), resolution=resolution,
                    marching_cubes_bound=bound.tolist(), level_set=0)
    device = opt._device
    mesh = mesher.get_mesh(device, opt._ray_sampler, skip_step=1)
    if mesh is None:
        print("map against the ground-truth mesh: the trained map has no surface to score")
        return
    os.makedirs(os.path.join(log, "meshes"), exist_ok=True)
    out = os.path.join(log, "meshes", f"mesh_{resolution}.ply")
    mesh.write_ply(out)
    score = evaluate_mesh_to_mesh(mesh, gt_mesh, device=device)
    print(f"mesh: {mesh.triangles.shape[0]} triangles written to {out}")
    print("map against the ground-truth mesh (exact distances, m; shares at 0.1 m): " +
          ", ".join(f"{k} {score[k]:.4f}" for k in ("accuracy", "completion", "chamfer", "precision", "recall", "f_score")))


def reread_scans(files, stamps, fov, device):
    """The scan files once more, as the run ingested them (build_scan_from_points: directions, ranges, absolute fp32 times)"""
    scans = []
    for path, stamp in zip(files, stamps):
        points = np.load(path)
        scan, _ = build_scan_from_points(points[:, :3].astype(np.float32), points[:, 3], float(stamp), fov=fov)
        scans.append(scan.to(device))
    return scans


def pose_graph_refine(files, stamps, fov, device, log, args):
    """Multiway registration of the scans along estimated_trajectory.txt -> trajectory/pose_graph_trajectory.txt"""
    from loner_amd.analysis.pose_graph import refine_trajectory
    est = os.path.join(log, "trajectory", "estimated_trajectory.txt")
    out = os.path.join(log, "trajectory", "pose_graph_trajectory.txt")
    rows = read_tum(est)
    scan_idx, row_idx = associate(stamps, rows[:, 0], t_max_diff=1e-3)
    scans = reread_scans([files[k] for k in scan_idx], stamps[scan_idx], fov, device)
    info = {}
    refine_trajectory(scans, rows[row_idx], out, args.pose_graph_distance, args.loop_radius, args.loop_gap, args.icp_estimation,
                      voxel_size=0.1, info=info)
    edges = info["edges"]
    print(f"pose graph: {len(scans)} nodes, {sum(e['added'] for e in edges)} of {len(edges)} edges added "
          f"({sum(e['added'] and e['uncertain'] for e in edges)} loop candidates), {len(info['pruned'])} pruned; "
          f"{info['first']['trials']} + {info['second']['trials']} trials, stops {info['first']['stop_reason']} / {info['second']['stop_reason']}")
    print(f"pose graph trajectory: {out}")
    if args.gt:
        score = ape(out, args.gt)
        print("APE after the pose graph (aligned, m): " + ", ".join(f"{k} {score[k]:.4f}" for k in ("rmse", "mean", "median", "std", "min", "max")))


def tsdf_baseline(what, tag, scans, trajectory, gt_mesh_path, resolution, log, device, sparse=False):
    """Fuse the scans along a trajectory (a TUM file) into a TSDF volume over the neural mesh's box, mesh it at the same resolution,
    write it beside the neural mesh and print the same evaluate_mesh_to_mesh line; sparse: a SparseTSDFVolume over the same box"""
    from loner_amd.analysis.mesh_eval import evaluate_mesh_to_mesh
    from loner_amd.analysis.mesher import TriangleMesh
    from loner_amd.analysis.tsdf import fuse_scans
    gt_mesh = TriangleMesh.read_ply(gt_mesh_path)
    bound = (gt_mesh.vertices.min(axis=0) - 1.0, gt_mesh.vertices.max(axis=0) + 1.0)
    stats = {}
    volume = fuse_scans(scans, trajectory, bound, resolution, device=device, stats=stats, sparse=sparse)
    print(f"TSDF on the {what}: {stats['scans'] - stats['skipped_scans']} of {stats['scans']} scans fused (a scan whose sweep leaves "
          f"the trajectory's time span is left out), {stats.get('node_updates', 0)} node updates" +
          (f", {volume.n_blocks} blocks of 8 x 8 x 8 nodes ({volume.memory_bytes() / 2 ** 20:.1f} MiB in blocks, "
           f"{volume.allocated_bytes() / 2 ** 20:.1f} MiB allocated)" if sparse else ""))
    mesh = volume.extract_mesh()
    if mesh is None:
        print(f"TSDF on the {what} against the ground-truth mesh: the volume has no surface to score")
        return
    os.makedirs(os.path.join(log, "meshes"), exist_ok=True)
    out = os.path.join(log, "meshes", f"tsdf_{tag}_{resolution}.ply")
    mesh.write_ply(out)
    score = evaluate_mesh_to_mesh(mesh, gt_mesh, device=device)
    print(f"mesh: {mesh.triangles.shape[0]} triangles written to {out}")
    print(f"TSDF on the {what} against the ground-truth mesh (exact distances, m; shares at 0.1 m): " +
          ", ".join(f"{k} {score[k]:.4f}" for k in ("accuracy", "completion", "chamfer", "precision", "recall", "f_score")))


if __name__ == "__main__":
    main()
