"""Camera rendering on the MI355X: lnr_build_camera_rays against the reference's capture (G17), lnr_render_forward_peak bit for bit
against lnr_render_forward and torch.argmax of the weights it writes, Model.render_depth_peak against forward(testing=True),
DepthRenderer.render_frame / render_stills on a small trained synthetic map, and lnr_depth_colormap against the numpy restatement
(tests/camera_restatement.py)."""
import os

import numpy as np
import pytest
import torch

from tests import camera_restatement as CM

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _calibration(h, w, k):
    from loner_amd.common.settings import Settings
    k = torch.as_tensor(k, dtype=torch.float32)
    return Settings({"camera_intrinsic": {"width": w, "height": h, "k": k, "new_k": k.clone(), "distortion": torch.zeros(4)},
                     "lidar_to_camera": {"xyz": [0.0, 0.0, 0.0], "orientation": [0.5, -0.5, 0.5, -0.5]}})


# ---------------------------------------------------------------- rays
def test_camera_rays_match_the_reference_capture():
    from loner_amd.common.pose import Pose
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.ray_utils import CameraRayDirections
    g = CM.g17()
    h, w = int(g["height"]), int(g["width"])
    crd = CameraRayDirections(_calibration(h, w, g["k"]), chunk_size=h * w)
    assert crd.directions.is_cuda and np.array_equal(crd.directions.cpu().numpy().view(np.uint32), g["directions"].view(np.uint32))
    wc = WorldCube(torch.tensor(float(g["scale"])), torch.from_numpy(g["shift"]))
    rr = torch.from_numpy(g["ray_range"])
    worst = 0.0
    for i in range(3):
        T = torch.from_numpy(g[f"T{i}"])
        pose = Pose(T.clone())
        rays = crd.fetch_chunk_rays(0, pose, wc, rr)
        assert torch.equal(pose.get_transformation_matrix(), T)                   # the caller's pose is not modified
        got, want = rays.cpu().numpy(), g[f"rays{i}"]
        assert got.shape == want.shape
        for lo, hi in ((0, 3), (3, 9), (9, 11), (11, 12), (12, 13)):
            worst = max(worst, CM.rel_err(got[:, lo:hi], want[:, lo:hi]))
        assert np.array_equal(got[:, 9:11], want[:, 9:11])
        whole, none = crd.build_rays(None, pose, None, wc, rr)                    # all rays, in order
        assert none is None and _same_bits(whole, rays)
        assert _same_bits(crd.fetch_chunk_rays(0, pose, wc, rr), rays)            # bit-identical from run to run
        idx = torch.from_numpy(g["scattered"])
        assert _same_bits(crd.build_rays(idx, pose, None, wc, rr)[0], rays[idx.to(DEV)])       # scattered indices: the same records
    pose = Pose(torch.from_numpy(g["T1"]))
    worst = max(worst, CM.rel_err(crd.build_rays(torch.from_numpy(g["scattered"]), pose, None, wc, rr)[0].cpu().numpy(), g["rays_scattered"]))
    print(f"lnr_build_camera_rays against G17: worst relative error {worst:.3g}")
    assert worst < 1e-6
    # a pose that requires grad is detached; intensities follow the indices; an index outside the image raises
    T = torch.from_numpy(g["T1"]).clone().requires_grad_(True)
    rays = crd.build_rays(None, Pose(T, fixed=False), None, wc, rr)[0]
    assert not rays.requires_grad and _same_bits(rays, crd.build_rays(None, pose, None, wc, rr)[0])

    class _Image:
        image = torch.arange(h * w * 3, dtype=torch.float32).reshape(h, w, 3)
    idx = torch.tensor([5, 0, 191])
    _, inten = crd.build_rays(idx, pose, _Image(), wc, rr)
    assert torch.equal(inten, _Image.image.reshape(-1, 3)[idx])
    with pytest.raises(IndexError):
        crd.build_rays(torch.tensor([0, h * w]), pose, None, wc, rr)


def test_camera_rays_of_an_image_that_is_no_multiple_of_the_block():
    """37 x 53 = 1961 rays (7 full blocks of 256 and a ragged one), chunks of 512: against the torch restatement at 1e-6"""
    from loner_amd.common.pose import Pose
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.ray_utils import CameraRayDirections
    h, w = 37, 53
    crd = CameraRayDirections(_calibration(h, w, [[40.0, 0.0, 26.0], [0.0, 41.0, 18.0], [0.0, 0.0, 1.0]]))
    wc = WorldCube(torch.tensor(42.5), torch.tensor([1.5, -2.0, 0.75]))
    pose = Pose(pose_tensor=torch.tensor([3.0, -4.5, 1.25, 0.3, -0.7, 1.9]))
    T = pose.get_transformation_matrix()
    rays = crd.build_rays(None, pose, None, wc, [1.0, 50.0])[0]
    assert rays.shape == (h * w, 13) and bool(torch.isfinite(rays).all())
    want = CM.camera_rays(crd.directions.cpu(), None, w, T, 1.0, 42.5, [1.5, -2.0, 0.75]).numpy()
    got = rays.cpu().numpy()
    for lo, hi in ((0, 3), (3, 9), (9, 11), (11, 12), (12, 13)):
        assert CM.rel_err(got[:, lo:hi], want[:, lo:hi]) < 1e-6
    assert np.array_equal(got[:, 9], np.arange(h * w) % w) and np.array_equal(got[:, 10], np.arange(h * w) // w)
    assert crd.num_chunks == 4
    chunks = torch.cat([crd.fetch_chunk_rays(c, pose, wc, [1.0, 50.0]) for c in range(crd.num_chunks)])
    assert _same_bits(chunks, rays)


# ---------------------------------------------------------------- the peak kernel
def _peak_inputs(n, S, seed):
    """seeded sigma / z / rays; with n >= 6 the first rows are planted: 0 all sigma <= 0, 1 the maximum in the last sample, 2 / 3 the
    maximum at a lane's first / last sample, 4 a NaN sigma, 5 a spike at sample 0"""
    gen = torch.Generator().manual_seed(seed)
    C = 1
    while 64 * C < S:
        C *= 2
    rays = torch.zeros(n, 13)
    rays[:, 0:3] = torch.rand(n, 3, generator=gen) * 0.2 - 0.1
    d = torch.randn(n, 3, generator=gen)
    rays[:, 3:6] = d / d.norm(dim=1, keepdim=True)
    rays[:, 6:9] = -rays[:, 3:6]
    rays[:, 11], rays[:, 12] = 0.02, 0.9 + 0.2 * torch.rand(n, generator=gen)
    z = torch.sort(rays[:, 11:12] + (rays[:, 12:13] - rays[:, 11:12]) * torch.rand(n, S, generator=gen), dim=1).values
    sigma = torch.randn(n, S, generator=gen) * 30.0 + 5.0
    planted = {}
    if n >= 6:
        lane = 5
        sigma[0] = -torch.rand(S, generator=gen)
        sigma[0, 3] = 0.0
        spots = {1: S - 1, 2: lane * C, 3: lane * C + C - 1, 5: 0}
        for row, i in spots.items():
            sigma[row] = 0.0
            sigma[row, i] = 1e6
        sigma[4, S // 3] = float("nan")
        planted = {0: 0, **spots}
    return sigma.to(DEV), z.to(DEV), rays.to(DEV), planted


@pytest.mark.parametrize("S", [64, 96, 512, 1024, 2048])
@pytest.mark.parametrize("n", [1, 5, 261])
def test_render_forward_peak_equals_render_forward_and_argmax(n, S):
    from loner_amd import ops
    sigma, z, rays, planted = _peak_inputs(n, S, 1000 * n + S)
    noise = torch.randn(n, S, generator=torch.Generator().manual_seed(S)).to(DEV)
    live = torch.tensor([max(1, n - 3)], device=DEV, dtype=torch.int32)
    for name, kw in (("no noise", {}), ("explicit noise", dict(noise=noise, noise_std=1.0)),
                     ("in-kernel noise", dict(noise_std=1.0, seed=1234567)), ("fewer live rays", dict(noise_std=1.0, seed=99, n_rays_dev=live))):
        depth, weights, opacity, variance = ops.render_forward(sigma, z, rays, want_weights=True, **kw)
        d2, o2, v2, pz, pi = ops.render_forward_peak(sigma, z, rays, **kw)
        assert _same_bits(d2, depth) and _same_bits(o2, opacity) and _same_bits(v2, variance), name
        m = int(live.item()) if "n_rays_dev" in kw else n
        want_z, want_i = CM.peak(weights[:m], z[:m])
        assert pi.dtype == torch.int32 and torch.equal(pi[:m].cpu().long(), want_i), name
        assert _same_bits(pz[:m], want_z), name
        assert not bool(pi[m:].any()) and not bool(pz[m:].any())                  # rays beyond the live count are not touched
        if name == "no noise":
            for row, i in planted.items():
                assert int(pi[row]) == i, (row, i, int(pi[row]))
            if planted:
                assert not bool(weights[0].any())                                 # every weight 0: the first index
        assert _same_bits(ops.render_forward_peak(sigma, z, rays, **kw)[3], pz)


def test_render_forward_peak_nan_weight_and_nullable_outputs():
    """A NaN depth makes NaN weights from that sample on: the lowest NaN index is the peak, as torch.argmax on the CPU has it"""
    from loner_amd import hip, ops
    sigma, z, rays, _ = _peak_inputs(6, 512, 3)
    z[2, 200] = float("nan")
    _, weights, _, _ = ops.render_forward(sigma, z, rays)
    assert bool(torch.isnan(weights[2]).any())
    _, _, _, pz, pi = ops.render_forward_peak(sigma, z, rays)
    want_z, want_i = CM.peak(weights, z)
    assert torch.equal(pi.cpu().long(), want_i) and int(pi[2]) == int(torch.isnan(weights[2]).nonzero()[0])
    assert _same_bits(pz, want_z)
    only = torch.zeros(6, device=DEV, dtype=torch.int32)
    hip.check(hip.load().lnr_render_forward_peak(hip._ptr(sigma), hip._ptr(z), hip._ptr(rays), 6, None, 512, None, 0.0, 0, None, None, None,
                                                 None, hip._ptr(only), hip._stream()))
    assert torch.equal(only, pi)


# ---------------------------------------------------------------- colour map
def test_depth_colormap_is_bit_identical_to_the_restatement():
    from loner_amd import ops
    from loner_amd.analysis.renderer import depth_to_rgba
    from loner_amd.analysis.turbo import turbo_u8
    img = CM.colour_image(37, 53)
    table = torch.from_numpy(turbo_u8()).to(DEV)
    dimg = torch.from_numpy(img).to(DEV)
    for mult, lo, hi in ((1.0, 1, 50), (1.0, 1, 75), (42.5, 1, 50), (0.37, 0.5, 12.25)):
        got = ops.depth_colormap(dimg, table, mult, lo, hi)
        assert got.shape == (37, 53, 4) and got.dtype == torch.uint8
        want = CM.depth_colormap(img, turbo_u8(), mult, lo, hi)
        assert np.array_equal(got.cpu().numpy(), want), (mult, lo, hi, int((got.cpu().numpy() != want).any(-1).sum()))
    assert np.array_equal(depth_to_rgba(dimg.reshape(1, 1, 37, 53), max_depth=75).cpu().numpy(), CM.depth_colormap(img, turbo_u8(), 1.0, 1, 75))
    with pytest.raises(ValueError):
        ops.depth_colormap(dimg, table, 1.0, 5, 5)


# ---------------------------------------------------------------- a trained map
H, W = 24, 32
K_SMALL = [[20.0, 0.0, 15.5], [0.0, 20.0, 11.5], [0.0, 0.0, 1.0]]


@pytest.fixture(scope="module")
def trained():
    """one synthetic keyframe (box room + sphere) trained for 150 iterations with the default settings: the recipe of
    tests/test_gpu_lidar_map.py; rendered here at 512 samples per ray"""
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from tests.test_gpu_lidar_map import _world_cube
    from tests.test_gpu_mapping import make_keyframes
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    wc = _world_cube()
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(150, True, False, False, True))
    opt._model.cfg["render"]["N_samples_test"] = 512          # (item access: attribute access may hand out a copy of a nested dict)
    assert opt._model._sample_counts(True)[0] == 512
    return opt, wc


def _renderer(trained, ckpt=None):
    from loner_amd.analysis.renderer import DepthRenderer
    opt, wc = trained
    return DepthRenderer(opt._model, ckpt or {"poses": []}, wc, torch.tensor([1.0, 50.0]), _calibration(H, W, K_SMALL))


@pytest.mark.parametrize("launches", [1, 3])
def test_render_depth_peak_equals_forward(trained, launches):
    from loner_amd.common.pose import Pose
    from loner_amd.utils import synthetic as SY
    opt, wc = trained
    model, sampler = opt._model, opt._ray_sampler
    r = _renderer(trained)
    cam = r.camera_pose(Pose(pose_tensor=SY.trajectory_pose6(3)[2].clone())).to(DEV)
    rays = r.ray_directions.build_rays(None, cam, None, wc, r.ray_range)[0]
    assert rays.shape == (H * W, 13)
    if launches > 1:
        model._POINTS_PER_LAUNCH = (H * W // launches) * 512                    # 256 rays per launch
    try:
        torch.manual_seed(11)
        with torch.no_grad():
            out = model(rays, sampler, wc.scale_factor, testing=True, camera=False)
        torch.manual_seed(11)
        depth, peak = model.render_depth_peak(rays, sampler)
        torch.manual_seed(11)
        again = model.render_depth_peak(rays, sampler)
    finally:
        if launches > 1:
            del model._POINTS_PER_LAUNCH
    assert out["weights_fine"].shape == (H * W, 512)
    want_peak, idx = CM.peak(out["weights_fine"], out["samples_fine"])
    assert _same_bits(depth, out["depth_fine"]) and _same_bits(peak, want_peak)
    assert _same_bits(again[0], depth) and _same_bits(again[1], peak)
    assert len(torch.unique(idx)) > 20                                            # a trained map: the peaks are spread along the rays
    assert model.render_depth_peak(rays[:0], sampler)[1].shape == (0,)


def test_render_frame_shapes_units_and_consistency(trained):
    from loner_amd.analysis.renderer import DepthRenderer
    from loner_amd.common.pose import Pose
    from loner_amd.utils import synthetic as SY
    opt, wc = trained
    model, sampler = opt._model, opt._ray_sampler
    r = _renderer(trained)
    cam = r.camera_pose(Pose(pose_tensor=SY.trajectory_pose6(2)[1].clone())).to(DEV)
    torch.manual_seed(5)
    depth, cons = r.render_frame(cam, sampler)
    assert depth.shape == cons.shape == (1, 1, H, W) and depth.is_cuda
    rays = r.ray_directions.build_rays(None, cam, None, wc, r.ray_range)[0]
    torch.manual_seed(5)
    d, p = model.render_depth_peak(rays, sampler)
    scale = wc.scale_factor.to(DEV).float()
    assert _same_bits(depth.reshape(-1), d * scale)                               # metres
    assert _same_bits(cons.reshape(-1), (p - d).abs() * scale)
    # the synthetic room: the camera looks along the lidar's x axis at a wall 20 m away (a ray through the window may run on to
    # the cube's wall: far is not capped by the sensor range)
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(cons).all()) and float(cons.min()) >= 0.0
    assert 1.0 < float(depth.median()) < 50.0
    torch.manual_seed(5)
    only, none = r.render_frame(cam, sampler, consistency=False)
    assert none is None and _same_bits(only, depth)
    outside = Pose(pose_tensor=torch.tensor([500.0, 0.0, 0.0, 0.0, 0.0, 0.0])).to(DEV)
    with pytest.raises(AssertionError, match="outside the world cube"):
        r.render_frame(outside, sampler)
    # the lidar-only default camera (not rendered here: 196 608 rays)
    default = DepthRenderer(model, {"poses": []}, wc, torch.tensor([1.0, 50.0]))
    assert default.im_size == (384, 512) and len(default.ray_directions) == 384 * 512
    want = torch.tensor([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    assert float((default.lidar_to_camera.get_transformation_matrix()[:3, :3] - want).abs().max()) < 1e-6


def test_render_stills_writes_the_colour_mapped_depth(trained, tmp_path):
    from loner_amd.analysis.renderer import depth_to_rgba
    from loner_amd.common.pose import Pose
    from loner_amd.utils import synthetic as SY
    opt, wc = trained
    sampler = opt._ray_sampler
    poses6 = SY.trajectory_pose6(3)
    ckpt = {"poses": [{"lidar_pose": poses6[i].clone(), "gt_lidar_pose": poses6[i + 1].clone(), "timestamp": torch.tensor(12.3456 + i)}
                      for i in range(2)]}
    r = _renderer(trained, ckpt)
    torch.manual_seed(3)
    paths = r.render_stills(sampler, tmp_path / "renders", skip_step=1)
    assert [os.path.basename(p) for p in paths] == ["predicted_depth_12_34.png", "predicted_depth_13_34.png"]
    torch.manual_seed(3)
    for i, path in enumerate(paths):
        cam = r.camera_pose(Pose(pose_tensor=poses6[i].clone())).to(DEV)
        depth, _ = r.render_frame(cam, sampler, consistency=False)
        want = depth_to_rgba(depth, max_depth=75).cpu().numpy()
        assert want.shape == (H, W, 4) and np.array_equal(CM.read_png(path), want)
        assert len(np.unique(want.reshape(-1, 4), axis=0)) > 10                   # an image, not one colour
    torch.manual_seed(3)
    last = r.render_stills(sampler, tmp_path / "gt", use_gt_poses=True, only_last_frame=True)
    assert [os.path.basename(p) for p in last] == ["predicted_depth_13_34.png"]
    torch.manual_seed(3)
    cam = r.camera_pose(Pose(pose_tensor=poses6[2].clone())).to(DEV)
    assert np.array_equal(CM.read_png(last[0]), depth_to_rgba(r.render_frame(cam, sampler, consistency=False)[0], max_depth=75).cpu().numpy())
    assert r.render_stills(sampler, tmp_path / "none", skip_step=15, start_frame=2) == []


def test_render_flythrough_writes_numbered_frames(trained, tmp_path):
    """Two trajectory poses taken as they are (interpolate=False, in the global frame): one numbered frame per pose, coloured over
    [1, max_depth], and no spin indices; with render_global=False the first frame is rendered from the identity."""
    from loner_amd.analysis.renderer import depth_to_rgba, flythrough_poses
    from loner_amd.common.pose import Pose
    opt, wc = trained
    sampler = opt._ray_sampler
    r = _renderer(trained)
    rows = np.array([[0.0, 0.5, -1.0, 0.25, 0.0, 0.0, 0.0, 1.0],
                     [0.1, 1.5, 0.5, 0.0, 0.0, 0.0, np.sin(0.2), np.cos(0.2)]])           # the second: 0.4 rad about z
    torch.manual_seed(8)
    paths, spins = r.render_flythrough(rows, sampler, tmp_path / "fly", render_global=True, interpolate=False, max_depth=40)
    assert [os.path.basename(p) for p in paths] == ["flythrough_depth_00000.png", "flythrough_depth_00001.png"] and spins == []
    poses, _ = flythrough_poses(rows, render_global=True, interpolate=False)
    assert poses.dtype == torch.float32 and tuple(poses.shape) == (2, 4, 4)
    assert torch.equal(poses[0], torch.tensor([[1.0, 0, 0, 0.5], [0, 1.0, 0, -1.0], [0, 0, 1.0, 0.25], [0, 0, 0, 1.0]]))
    assert abs(float(poses[1, 1, 0]) - np.sin(0.4)) < 1e-7 and poses[1, :3, 3].tolist() == [1.5, 0.5, 0.0]
    torch.manual_seed(8)
    frames = []
    for pose, path in zip(poses, paths):
        depth, _ = r.render_frame(r.camera_pose(Pose(pose)).to(DEV), sampler, consistency=False)
        want = depth_to_rgba(depth, max_depth=40).cpu().numpy()
        frames.append(want)
        assert np.array_equal(CM.read_png(path), want)
    assert not np.array_equal(frames[0], frames[1])
    torch.manual_seed(8)
    rel, _ = r.render_flythrough(rows, sampler, tmp_path / "rel", interpolate=False, max_depth=40)
    torch.manual_seed(8)
    depth, _ = r.render_frame(r.camera_pose(Pose(torch.eye(4))).to(DEV), sampler, consistency=False)
    assert np.array_equal(CM.read_png(rel[0]), depth_to_rgba(depth, max_depth=40).cpu().numpy())
