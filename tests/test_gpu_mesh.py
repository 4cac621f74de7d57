"""Meshing on the MI355X: lnr_render_mesh_accumulate against the CPU restatement of the reference's accumulation, lnr_mc_* against the
numpy marching cubes, and Mesher.get_mesh end to end on a map trained on the synthetic scene."""
import numpy as np
import pytest
import torch

from tests import mesh_restatement as MR

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _world_cube():
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.utils import synthetic as SY
    scale, shift = SY.world_cube()
    return WorldCube(torch.tensor(scale), torch.from_numpy(shift))


def _lattice(mcb, resolution, wc):
    """Mesher's lattice (axes + bound) for a marching_cubes_bound in metres"""
    from loner_amd import ops
    from loner_amd.analysis.mesher import Mesher
    m = Mesher(None, {"poses": []}, wc, torch.tensor([1.0, 50.0]), resolution=resolution, marching_cubes_bound=mcb)
    axes = m.get_grid_uniform(resolution)["xyz"]
    bound = torch.from_numpy(m._bound())
    return ops.MeshLattice(axes, bound.numpy(), DEV), axes, bound


def _scan_rays(n_rays, wc, pose_index=2):
    from loner_amd.common.pose import Pose
    from loner_amd.common.ray_utils import LidarRayDirections
    from loner_amd.common.sensors import LidarScan
    from loner_amd.utils import synthetic as SY
    from oracle import poses as OP
    dirs, ts = SY.lidar_pattern()
    pose6 = SY.trajectory_pose6(4)[pose_index]
    sub = torch.arange(3, dirs.shape[1], 7)[:n_rays]
    scan = LidarScan(dirs[:, sub].clone(), SY.scene_ranges(dirs, OP.transform_from_pose6(pose6))[sub], ts[sub])
    lrd = LidarRayDirections(scan, chunk_size=len(sub))
    return lrd.fetch_chunk_rays(0, Pose(pose_tensor=pose6.clone(), fixed=True), wc, torch.tensor([1.0, 50.0]))


@pytest.fixture(scope="module")
def trained():
    """one synthetic keyframe (box room + sphere) trained for 150 iterations with the default settings: a map with surfaces"""
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from tests.test_gpu_mapping import make_keyframes
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    wc = _world_cube()
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(150, True, False, False, True))
    return opt, wc


@pytest.mark.parametrize("n_samples,n_rays,var_filter,launch", [(512, 3001, False, None), (512, 3001, True, 1 << 20),
                                                                 (2048, 1203, False, None), (2048, 1203, True, 1 << 20)])
def test_accumulation_is_bit_identical_to_the_restated_reference(trained, n_samples, n_rays, var_filter, launch):
    """Model.mesh_accumulate vs the reference's sequence (restated with a scatter-max) fed by Model.forward(testing=False,
    return_variance=True) under the same torch seed, on a trained map: ragged ray counts, one launch and several (the sampler-ahead
    stream), with and without the variance filter (threshold near the median variance).  Bit for bit: the fused kernel composites
    with lnr_render_forward's render_ray and the same fma contractions (lnr_mesh.hip, top)."""
    opt, wc = trained
    model, sampler = opt._model, opt._ray_sampler
    render = model.cfg.render
    saved = (render["N_samples_train"], model._POINTS_PER_LAUNCH)
    render["N_samples_train"] = n_samples
    if launch is not None:
        model._POINTS_PER_LAUNCH = launch
    try:
        mcb = [[-19.5, 19.5], [-14.5, 14.5], [-1.9, 5.9]]
        lattice, axes, bound = _lattice(mcb, 0.5, wc)
        rays = _scan_rays(n_rays, wc, pose_index=0)
        assert rays.shape[0] == n_rays
        ray_range = torch.tensor([1.0, 50.0])
        torch.manual_seed(1234)
        with torch.no_grad():
            out = model(rays, sampler, wc.scale_factor, testing=False, return_variance=True, camera=False)
        var_threshold = None
        if var_filter:                      # half way across the widest gap between sorted variances near the median: no ray sits
            v = out["variance"].double().sort().values.cpu()        # within rounding of the threshold
            k = n_rays // 2 - 20 + int((v[n_rays // 2 - 19:n_rays // 2 + 21] - v[n_rays // 2 - 20:n_rays // 2 + 20]).argmax())
            var_threshold = float(0.5 * (v[k] + v[k + 1]))
        ref = torch.zeros(lattice.n_nodes, dtype=torch.float64)
        MR.restated_accumulate(ref, out["points_fine"].cpu(), out["weights_fine"].cpu(), out["depth_fine"].cpu(), out["variance"].cpu(),
                               bound, axes, ray_range, var_threshold)
        vol = torch.zeros(lattice.n_nodes, device=DEV)
        counters = torch.zeros(2, device=DEV, dtype=torch.int64)
        torch.manual_seed(1234)
        model.mesh_accumulate(rays, sampler, lattice, vol, float(ray_range[1]) - 0.25, var_threshold, counters=counters)
    finally:
        render["N_samples_train"], model._POINTS_PER_LAUNCH = saved
    got = vol.cpu().double()
    n_in, n_atomic = (int(x) for x in counters.cpu())
    n_valid = int((out["variance"] < var_threshold).sum()) if var_threshold is not None else n_rays
    print(f"S={n_samples} rays={n_rays} var<{var_threshold} ({n_valid} rays kept): {int((ref > 0).sum())} voxels hit, {n_in} samples "
          f"reached the volume, {n_atomic} atomics ({n_atomic / max(n_in, 1):.3f} per sample)")
    assert int((ref > 0).sum()) > 100 and 0 < n_valid < n_rays + (0 if var_filter else 1)
    differ = got != ref
    print(f"  voxels with other bits: {int(differ.sum())} of {int((ref > 0).sum())}")
    assert torch.equal(got, ref), f"{int(differ.sum())} voxels differ"


def test_accumulation_on_hand_placed_samples_hits_boundaries_and_aliasing_buckets():
    """Rays along the lattice axes whose sample depths put points exactly on nodes, on the fp32 bound and in (bound_hi, fp32(bound_hi)]
    (bucket n: the reference's flat index aliases into the next row), fed through ops.mesh_accumulate and ops.render_forward alike."""
    from loner_amd import ops
    wc = _world_cube()
    lattice, axes, bound = _lattice([[-3.0, 4.0], [-2.0, 3.0], [-1.5, 1.0]], 0.25, wc)
    b = bound.numpy()
    S, rays, zs = 64, [], []
    g = torch.Generator().manual_seed(5)
    for a in range(3):
        ax = axes[a]
        hi32 = np.float32(b[a][1])
        targets = np.concatenate([ax[:S // 2].astype(np.float32), [np.float32(b[a][0]), hi32, np.nextafter(hi32, np.float32(-1e9))]])
        for r in range(6):
            o = np.array([np.float32(axes[i][(3 * r + 1) % len(axes[i])]) for i in range(3)], dtype=np.float32)
            o[a] = np.float32(b[a][0] - 0.01)
            d = np.zeros(3, dtype=np.float32)
            d[a] = np.float32(1.0)
            # z with o + 1 * z == target in fp32 where possible (the sum is exact when o and the target share the binade range)
            z = np.sort((targets.astype(np.float64) - o[a]).astype(np.float32))
            z = np.concatenate([z, np.linspace(z[-1] + 1e-3, z[-1] + 0.2, S - len(z), dtype=np.float32)])[:S]
            rec = np.zeros(13, dtype=np.float32)
            rec[0:3], rec[3:6], rec[6:9], rec[11], rec[12] = o, d, d, 0.0, np.float32(1.0)
            rays.append(rec)
            zs.append(np.sort(z))
    rays = torch.from_numpy(np.stack(rays)).to(DEV)
    z = torch.from_numpy(np.stack(zs)).to(DEV)
    sigma = (torch.rand(z.shape, generator=g) * 40.0 - 5.0).to(DEV)
    depth, weights, _, variance = ops.render_forward(sigma, z, rays)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    ref = torch.zeros(lattice.n_nodes, dtype=torch.float64)
    MR.restated_accumulate(ref, pts.cpu(), weights.cpu(), depth.cpu(), variance.cpu(), bound, axes, torch.tensor([1.0, 50.0]))
    vol = torch.zeros(lattice.n_nodes, device=DEV)
    ops.mesh_accumulate(sigma, z, rays, lattice, vol, 49.75)
    # the fixture reaches the aliasing bucket on some axis
    p = pts.reshape(-1, 3).cpu()
    alias = False
    for a in range(3):
        ok = (p[:, a] >= bound[a][0]) & (p[:, a] <= bound[a][1])
        alias = alias or bool((torch.bucketize(p[ok, a], torch.from_numpy(axes[a])) == len(axes[a])).any())
    assert alias
    assert int((ref > 0).sum()) > 50
    assert torch.equal(vol.cpu().double(), ref), f"{int((vol.cpu().double() != ref).sum())} voxels differ"


def _mc_both(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    from loner_amd import ops
    verts, faces = ops.marching_cubes(vol, level, spacing, origin)
    rv, rf = MR.marching_cubes(vol.cpu().numpy(), level, ops.mc_case_table(), spacing, origin)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), "vertices differ"
    assert np.array_equal(f, rf), "triangles differ"
    return v, f


def test_marching_cubes_matches_the_numpy_restatement():
    ax = torch.arange(64, dtype=torch.float32, device=DEV)
    x, y, zz = torch.meshgrid(ax, ax, ax, indexing="ij")
    sphere = 25.3 ** 2 - ((x - 31.2) ** 2 + (y - 32.6) ** 2 + (zz - 30.9) ** 2)
    v, f = _mc_both(sphere.contiguous(), 0.0, spacing=(0.1, 0.2, 0.3), origin=(-1.0, 2.0, 0.5))
    assert MR.closed_and_oriented(f, len(v)) == (True, True) and MR.euler_characteristic(f) == 2
    g = torch.Generator(device=DEV).manual_seed(7)
    noise = torch.randn(97, 83, 71, device=DEV, generator=g)
    v, f = _mc_both(noise, 0.1)
    assert f.shape[0] > 100000


def test_marching_cubes_beyond_two_to_the_26_nodes():
    """69 M nodes: 16.8 k count blocks, so the block-offset scan runs 17 chunks with a carry"""
    nx, ny, nz = 420, 410, 400
    assert nx * ny * nz > 2 ** 26
    i = torch.arange(nx, device=DEV, dtype=torch.float32)[:, None, None]
    j = torch.arange(ny, device=DEV, dtype=torch.float32)[None, :, None]
    k = torch.arange(nz, device=DEV, dtype=torch.float32)[None, None, :]
    vol = 150.5 ** 2 - ((i - 201.3) ** 2 + (j - 205.1) ** 2 + (k - 198.7) ** 2)
    vol = vol + 40.0 * torch.sin(i * 0.3) * torch.cos(j * 0.2)
    v, f = _mc_both(vol.contiguous(), 0.0)
    assert MR.closed_and_oriented(f, len(v)) == (True, True)


def test_marching_cubes_empty_and_out_of_range_levels():
    from loner_amd import ops
    vol = torch.rand(17, 9, 12, device=DEV)
    for level in (2.0, -1.0):
        verts, faces = ops.marching_cubes(vol, level)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)
    verts, faces = ops.marching_cubes(torch.zeros(5, 6, 7, device=DEV), 0.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    with pytest.raises(RuntimeError):
        ops.marching_cubes(torch.zeros(1, 6, 7, device=DEV), 0.0)


def test_mesher_get_mesh_on_a_trained_synthetic_map(tmp_path):
    """Train one synthetic keyframe (box room 40 x 30 x 8 m with a sphere) for 300 iterations, then mesh it at 0.2 m and the reference's
    default level 0 (every voxel a positive weight reached is inside, so the surface sits at or in front of the walls).  First
    measurement: 244 841 vertices, 484 202 triangles; 22.2 % / 44.3 % / 66.6 % of the vertices within 0.25 / 0.5 / 1 m of the analytic
    surfaces; every open edge at the lattice bound.  Bounds: 35 % within 0.5 m, 55 % within 1 m."""
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from tests.test_gpu_mapping import make_keyframes
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    wc = _world_cube()
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(300, True, False, False, True))
    ckpt = {"poses": [kf.get_pose_state()]}
    mcb = [[-21.0, 21.0], [-16.0, 16.0], [-3.0, 7.0]]
    mesher = Mesher(opt._model, ckpt, wc, torch.tensor([1.0, 50.0]), resolution=0.2, marching_cubes_bound=mcb, level_set=0)
    torch.manual_seed(3)
    mesh = mesher.get_mesh(DEV, opt._ray_sampler, skip_step=1)
    assert mesh is not None and mesh.triangles.shape[0] > 1000
    v = mesh.vertices
    lo, hi = np.array(mcb)[:, 0], np.array(mcb)[:, 1]
    assert ((v >= lo - 1e-4) & (v <= hi + 1e-4)).all()
    # distance to the analytic surfaces: the six walls of the box and the sphere
    bmin, bmax = np.array(SY.BOX_MIN), np.array(SY.BOX_MAX)
    d_box = np.minimum(np.abs(v - bmin), np.abs(v - bmax)).min(1)
    d_sph = np.abs(np.linalg.norm(v - np.array(SY.SPHERE_C), axis=1) - SY.SPHERE_R)
    d = np.minimum(d_box, d_sph)
    frac = {t: float((d < t).mean()) for t in (0.25, 0.5, 1.0)}
    # closed away from the lattice boundary: edges used once all lie on triangles touching the bound
    e = MR.edges_of(mesh.triangles).astype(np.int64)
    n = len(v)
    und = np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1])
    u, cnt = np.unique(und, return_counts=True)
    open_edges = u[cnt != 2]
    ends = np.stack([open_edges // n, open_edges % n], 1)
    near_bound = ((np.abs(v[ends.reshape(-1)] - lo) < 0.25) | (np.abs(v[ends.reshape(-1)] - hi) < 0.25)).any(1)
    print(f"mesh: {len(v)} vertices, {mesh.triangles.shape[0]} triangles; within 0.25 / 0.5 / 1 m of the scene: "
          f"{frac[0.25]:.3f} / {frac[0.5]:.3f} / {frac[1.0]:.3f}; edges not shared by two triangles: {len(open_edges)}, "
          f"of them away from the bound: {int((~near_bound).sum()) // 2}")
    assert near_bound.all()
    assert frac[0.5] > 0.35 and frac[1.0] > 0.55
    mesh.compute_vertex_normals()
    path = str(tmp_path / "mesh.ply")
    mesh.write_ply(path)
    back = TriangleMesh.read_ply(path)
    assert np.array_equal(back.vertices, mesh.vertices) and np.array_equal(back.triangles, mesh.triangles)
    assert np.array_equal(back.vertex_normals, mesh.vertex_normals)
