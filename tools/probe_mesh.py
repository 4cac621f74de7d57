"""Meshing costs (profiles/mesh_extraction.txt): per pose of Mesher.get_mesh (180 x 1440 rays x 512 samples, default network) the
forward-only render without weights against the fused render + weight accumulation, and the atomics issued per sample; marching
cubes at the canteen box (60 x 75 x 23 m, cfg/fusion_portable/canteen.yaml of the reference) at 0.1 m and 0.2 m by pass; the numpy
restatement on the same volumes for scale.

    python tools/probe_mesh.py [--out FILE] [--skip-numpy]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-numpy", action="store_true")
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis.mesher import Mesher, build_lidar_scan
    from loner_amd.common.pose import Pose
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.ray_utils import LidarRayDirections
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.models.model_tcnn import Model, OccupancyGridModel
    from loner_amd.models.ray_sampling import OccGridRaySampler
    from loner_amd.utils import synthetic as SY
    from tests import mesh_restatement as MR
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc = default_optimizer_settings().model_config.model
    model = Model(mc).to(dev)
    occ = OccupancyGridModel(mc.occ_model).to(dev)
    sig = model.nerf_model._model_sigma
    n_mlp, H = int(sig.spec.n_mlp_params), int(sig.spec.n_neurons)
    with torch.no_grad():                                    # trained-like: large table entries, a density that saturates at surfaces
        sig.params[n_mlp:] *= 3000.0
        sig.params[n_mlp - 16 * H:n_mlp - 15 * H] *= 300.0
        occ.occupancy_grid.copy_(torch.randn(occ.occupancy_grid.shape, generator=torch.Generator().manual_seed(1)).to(dev) * 2.0)
    sampler = OccGridRaySampler()
    sampler.update_occ_grid(occ().detach())
    scale, shift = SY.world_cube()
    wc = WorldCube(torch.tensor(scale), torch.from_numpy(shift))
    rr = torch.tensor([1.0, 50.0])
    canteen = [[-35, 25], [-30, 45], [-3, 20]]
    n_samples = int(mc.render.N_samples_train)
    say(f"# meshing costs on one MI355X; default network, N_samples_train = {n_samples}, trained-like parameters (tables x3000)")
    lrd = LidarRayDirections(build_lidar_scan({"vertical_fov": [-22.5, 22.5], "vertical_resolution": 0.25, "horizontal_resolution": 0.25}, dev))
    pose = Pose(pose_tensor=SY.trajectory_pose6(2)[1].clone(), fixed=True).to(dev)
    rays = lrd.build_lidar_rays(torch.arange(len(lrd)), rr, wc, pose.get_transformation_matrix())[0]
    say(f"pose: {rays.shape[0]} rays x {n_samples} samples = {rays.shape[0] * n_samples / 1e6:.1f} M samples")
    for res in (0.2, 0.1):
        m = Mesher(model, {"poses": []}, wc, rr, resolution=res, marching_cubes_bound=canteen)
        lattice = ops.MeshLattice(m.get_grid_uniform(res)["xyz"], m._bound(), dev)
        vol = torch.zeros(lattice.n_nodes, device=dev)
        t_render = timed(lambda: model._render_no_grad(rays, sampler, n_samples, float(mc.render.perturb), want_weights=False), 5)
        # every timed call accumulates into a zeroed volume (a filled one would let the skip-if-not-larger filter drop most atomics);
        # the zeroing is timed on its own and subtracted
        t_zero = timed(lambda: vol.zero_(), 5)
        t_fused = timed(lambda: (vol.zero_(), model.mesh_accumulate(rays, sampler, lattice, vol, 49.75)), 5) - t_zero
        vol.zero_()
        cnt = torch.zeros(2, device=dev, dtype=torch.int64)
        model.mesh_accumulate(rays, sampler, lattice, vol, 49.75, counters=cnt)
        n_in, n_at = (int(x) for x in cnt.cpu())
        n_all = rays.shape[0] * n_samples
        say(f"\n## lattice {lattice.shape} at {res} m ({lattice.n_nodes / 1e6:.1f} M nodes)")
        say(f"render alone (forward-only, no weights): {t_render:.2f} ms per pose")
        say(f"render + accumulate (fused):             {t_fused:.2f} ms per pose  (+{100 * (t_fused / t_render - 1):.1f} %), into a zeroed "
            f"volume each time (the zeroing, {t_zero:.3f} ms, subtracted)")
        say(f"samples reaching the volume {n_in} ({n_in / n_all:.3f} of all), atomics issued {n_at} "
            f"({n_at / n_all:.4f} per sample, {n_at / max(n_in, 1):.4f} per in-volume sample)")
        volume = vol.view(lattice.shape[1], lattice.shape[0], lattice.shape[2]).permute(1, 0, 2).contiguous()
        ops.profile_enable(True)
        ops.profile_read()
        reps = 5
        for _ in range(reps):
            verts, faces = ops.marching_cubes(volume, 0.0)
        torch.cuda.synchronize()
        prof = ops.profile_read()
        ops.profile_enable(False)
        t_mc = timed(lambda: ops.marching_cubes(volume, 0.0), reps)
        parts = ", ".join(f"{k} {v['total_ms'] / reps:.3f} ms" for k, v in prof.items() if k.startswith("mc_"))
        say(f"marching cubes: {verts.shape[0]} vertices, {faces.shape[0]} triangles; {t_mc:.2f} ms per call incl. the totals read-back "
            f"({parts})")
        if not args.skip_numpy:
            host = volume.cpu().numpy()
            table = ops.mc_case_table()
            t0 = time.perf_counter()
            rv, rf = MR.marching_cubes(host, 0.0, table)
            t1 = time.perf_counter()
            same = np.array_equal(rv.view(np.uint32), verts.cpu().numpy().view(np.uint32)) and np.array_equal(rf, faces.cpu().numpy())
            say(f"numpy restatement on the same volume: {1000 * (t1 - t0):.0f} ms (identical output: {same})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
