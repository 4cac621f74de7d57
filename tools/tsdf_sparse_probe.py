"""Sparse TSDF costs (profiles/tsdf_sparse.txt) on the room of tools/tsdf_probe.py (utils/synthetic_mesh.scene_mesh, 0.1 m, the scene's
box grown by 1 m): twelve simulated 64 x 1024 and 128 x 2048 sweeps, band only and carving, fused into a SparseTSDFVolume; the first
sweep (every block new) and the twelfth again (steady state: no block new) split into touch, insert and integrate, beside
ops.tsdf_integrate on the same rays in the same run; blocks, bytes and occupancy against the dense volume; the sparse field and marching
cubes against the dense ones; the sweeps replayed along a line across a lattice the dense volume refuses; and both volumes' meshes of
the twelve-sweep sequence scored against the scene.

    python tools/tsdf_sparse_probe.py [--out FILE] [--voxel 0.1]

Phases: host clock between device synchronisations (tsdf_sparse.sparse_tsdf_integrate(timings=...)); a phase includes the host read that ends
it, which the dense call does not have.  Steady state and the dense call: median (minimum) of 9 after 2 warm-up calls; the dense call
by device events around the call, and by the host clock with a synchronisation as the sparse phases are taken.  A first sweep is
measured once.
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mesh_distance_probe import wall  # noqa: E402
from tools.raycast_probe import timed  # noqa: E402


def host_timed(fn, reps=9, warm=2):
    """(median ms, min ms) of single calls by the host clock, the device idle before and after"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--voxel", type=float, default=0.1)
    args = ap.parse_args()
    from examples.simulate_sequence import default_trajectory
    from loner_amd import ops
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis import tsdf_sparse as SP
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.mesh_eval import evaluate_mesh_to_mesh
    from loner_amd.analysis.mesher import TriangleMesh
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.analysis.tsdf import SparseTSDFVolume, TSDFVolume, fuse_scans
    from loner_amd.utils import synthetic as SY
    from loner_amd.utils import synthetic_mesh as SM
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    v = args.voxel
    vertices, triangles = SM.scene_mesh()
    scene = RaycastingScene(vertices, triangles, device=dev)
    bound = (vertices.min(axis=0) - 1.0, vertices.max(axis=0) + 1.0)
    rows = default_trajectory(12, 0.1)
    traj = load_trajectory(rows, dev)
    dense_probe = TSDFVolume(*bound, v, device=dev)
    dense_bytes = 12 * int(np.prod(dense_probe.dims))
    say(f"# python tools/tsdf_sparse_probe.py --voxel {v}")
    say(f"# sparse TSDF on one MI355X ({torch.cuda.get_device_name(0)}); phases by the host clock between device synchronisations, each with")
    say("# the host read that ends it; steady state and dense: median (minimum) ms of 9 calls after 2 warm-up calls")
    say(f"lattice: {' x '.join(map(str, dense_probe.dims))} = {np.prod(dense_probe.dims) / 1e6:.1f} M nodes at {v} m, dense {dense_bytes / 2 ** 20:.0f} MiB")
    del dense_probe
    sweeps = {}
    for beams, azimuths in ((64, 1024), (128, 2048)):
        d, times = SY.lidar_pattern(beams, azimuths)
        batch = []
        for k in range(12):
            scan, _ = lidar_sim.simulate_scan(scene, traj, d.to(dev), times.to(dev), 0.1 * k, (1.0, 50.0), 0.0, k)
            rays, _ = ops.trajectory_rays(scan.ray_directions, scan.timestamps.double(), traj)
            keep = torch.isfinite(rays).all(dim=1)                       # (a sweep that leaves the trajectory's span loses those rays)
            batch.append((rays[keep].contiguous(), scan.distances.double()[keep].contiguous()))
        batch = [b for b in batch if 2 * b[0].shape[0] >= beams * azimuths]    # (a sweep that mostly leaves the trajectory's span is left out)
        sweeps[(beams, azimuths)] = batch
        warm = SparseTSDFVolume(*bound, v, device=dev)                       # (the first launches of the kernels are not a sweep's cost)
        warm.integrate_rays(*batch[0])
        del warm
        for what, front in (("band only", None), ("carving", math.inf)):
            vol = SparseTSDFVolume(*bound, v, front=front, device=dev)
            first, last = {}, {}
            for k, (rays, ranges) in enumerate(batch):
                t = first if k == 0 else last
                info = SP.sparse_tsdf_integrate(rays, ranges, vol.store, vol.dims, vol.origin, v, vol.sdf_trunc, vol.front, timings=t).cpu()
                assert int(info[7]) == 0
                if k == 0:
                    first_blocks = vol.n_blocks
            rays, ranges = batch[-1]
            n = rays.shape[0]
            say(f"{beams} x {azimuths}, {what}, {len(batch)} sweeps: sweep 1 ({batch[0][0].shape[0]} rays, {first['candidates']} candidates, {first_blocks} new blocks): "
                f"touch {first['touch']:.3f}, insert {first['insert']:.3f}, integrate {first['integrate']:.3f} ms; the last sweep "
                f"({n} rays, {last['candidates']} candidates, {int(info[5])} new blocks of {vol.n_blocks}): touch {last['touch']:.3f}, "
                f"insert {last['insert']:.3f}, integrate {last['integrate']:.3f} ms")
            steady = []
            for _ in range(11):
                t = {}
                SP.sparse_tsdf_integrate(rays, ranges, vol.store, vol.dims, vol.origin, v, vol.sdf_trunc, vol.front, timings=t)
                assert t["candidates"] == 0
                steady.append(t)
            steady = steady[2:]
            med = {key: statistics.median(t[key] for t in steady) for key in ("touch", "integrate")}
            low = {key: min(t[key] for t in steady) for key in ("touch", "integrate")}
            dense = TSDFVolume(*bound, v, front=front, device=dev)
            call = lambda: ops.tsdf_integrate(rays, ranges, dense.sum, dense.count, dense.origin, v, dense.sdf_trunc, dense.front)
            ev_med, ev_low = timed(call)
            host_med, host_low = host_timed(call)
            total = med["touch"] + med["integrate"]
            say(f"  steady state (the last sweep again): touch {med['touch']:.3f} ({low['touch']:.3f}), integrate {med['integrate']:.3f} "
                f"({low['integrate']:.3f}), together {total:.3f} ms; ops.tsdf_integrate on the same rays: {ev_med:.3f} ({ev_low:.3f}) ms by "
                f"device events, {host_med:.3f} ({host_low:.3f}) ms by the host clock: sparse / dense = {total / host_med:.2f} by the host "
                f"clock, {total / ev_med:.2f} against the events; {vol.n_blocks} blocks, {vol.memory_bytes() / 2 ** 20:.1f} MiB in blocks, "
                f"{vol.allocated_bytes() / 2 ** 20:.1f} MiB allocated")
            del dense, vol
    # memory and meshing on the twelve 64 x 1024 sweeps, band only
    batch = sweeps[(64, 1024)]
    vol, dense = SparseTSDFVolume(*bound, v, device=dev), TSDFVolume(*bound, v, device=dev)
    for rays, ranges in batch:
        vol.integrate_rays(rays, ranges)
        dense.integrate_rays(rays, ranges)
    field, valid = vol.field()
    observed = int(valid.sum())
    say(f"twelve 64 x 1024 sweeps, band only: {vol.n_blocks} blocks = {vol.memory_bytes() / 2 ** 20:.1f} MiB in blocks "
        f"({vol.allocated_bytes() / 2 ** 20:.1f} MiB allocated) against {dense_bytes / 2 ** 20:.0f} MiB dense; {observed} nodes observed: "
        f"{100.0 * observed / (512 * vol.n_blocks):.1f} % of the blocks' nodes, {100.0 * observed / np.prod(vol.dims):.2f} % of the lattice's")
    same = torch.equal(vol.to_dense()[0], dense.sum) and torch.equal(vol.to_dense()[1].view(torch.int32), dense.count.view(torch.int32))
    say(f"  to_dense() {'equals' if same else 'DIFFERS FROM'} the dense volume byte for byte")
    keys = vol.store.keys[:vol.n_blocks]
    a = timed(lambda: vol.field())
    b = timed(lambda: dense.field())
    say(f"  field + valid: sparse {a[0]:.3f} ({a[1]:.3f}) ms, dense {b[0]:.3f} ({b[1]:.3f}) ms")
    dfield, dvalid = dense.field()
    a = timed(lambda: SP.sparse_marching_cubes(keys, field, valid, vol.dims, 0.0, vol.spacing, vol.origin))
    b = timed(lambda: ops.marching_cubes(dfield, 0.0, dense.spacing, dense.origin, valid=dvalid))
    sv, sf = SP.sparse_marching_cubes(keys, field, valid, vol.dims, 0.0, vol.spacing, vol.origin)
    dv, df = ops.marching_cubes(dfield, 0.0, dense.spacing, dense.origin, valid=dvalid)
    say(f"  marching cubes: sparse {a[0]:.3f} ({a[1]:.3f}) ms, dense masked {b[0]:.3f} ({b[1]:.3f}) ms; {sv.shape[0]} vertices and "
        f"{sf.shape[0]} triangles against {dv.shape[0]} and {df.shape[0]}")
    # both meshes of the sequence against the scene (what the closed loop's TSDF lines score, along the ground truth)
    gt = TriangleMesh(vertices, triangles)
    d64, times64 = SY.lidar_pattern(64, 1024)
    for name, sparse in (("dense", False), ("sparse", True)):
        scans = [lidar_sim.simulate_scan(scene, traj, d64.to(dev), times64.to(dev), 0.1 * k, (1.0, 50.0), 0.0, k)[0] for k in range(12)]
        seconds, mesh = wall(lambda: fuse_scans(scans, rows, bound, v, device=dev, sparse=sparse).extract_mesh())
        score = evaluate_mesh_to_mesh(mesh, gt, device=dev)
        say(f"fuse_scans(sparse={sparse}) + extract_mesh, 12 sweeps of 64 x 1024 along the ground truth: {seconds * 1e3:.1f} ms by the host "
            f"clock, {mesh.triangles.shape[0]} triangles; against the scene's mesh (exact distances, m; shares at 0.1 m): " +
            ", ".join(f"{k} {score[k]:.4f}" for k in ("accuracy", "completion", "chamfer", "precision", "recall", "f_score")))
    del vol, dense, field, valid, dfield, dvalid
    # a scene the dense volume refuses: the sweeps replayed every 30 m along a diagonal of a 400 m x 400 m x 40 m lattice
    lo = np.asarray(bound[0])
    hi = lo + np.asarray([400.0, 400.0, 40.0])
    try:
        TSDFVolume(lo, hi, v, device=dev)
        refused = "does NOT refuse"
    except ValueError as e:
        refused = f"refuses ({e})"
    big = SparseTSDFVolume(lo, hi, v, device=dev)
    say(f"lattice {' x '.join(map(str, big.dims))} = {np.prod([float(n) for n in big.dims]) / 1e9:.2f} G nodes: TSDFVolume {refused}")
    per_sweep = []
    for k, (rays, ranges) in enumerate(batch):
        moved = rays.clone()
        moved[:, 0] += 30.0 * k
        moved[:, 1] += 30.0 * k
        t = {}
        info = SP.sparse_tsdf_integrate(moved, ranges, big.store, big.dims, big.origin, v, big.sdf_trunc, big.front, timings=t).cpu()
        assert int(info[7]) == 0
        per_sweep.append(t["touch"] + t["insert"] + t["integrate"])
    say(f"  twelve 64 x 1024 sweeps, each 30 m further along x and y, band only: {big.n_blocks} blocks, {big.memory_bytes() / 2 ** 20:.1f} MiB "
        f"in blocks ({big.allocated_bytes() / 2 ** 20:.1f} MiB allocated); per sweep, every block new: median "
        f"{statistics.median(per_sweep):.3f} ms, minimum {min(per_sweep):.3f}, maximum {max(per_sweep):.3f} (a sweep that grows the pool)")
    seconds, mesh = wall(lambda: big.extract_mesh(), warm=0)
    say(f"  extract_mesh: {seconds * 1e3:.1f} ms by the host clock, {0 if mesh is None else mesh.triangles.shape[0]} triangles")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
