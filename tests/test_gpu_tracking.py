"""The LiDAR tracker on the MI355X: the frame cloud against the reference's recorded arrays (G16), motion compensation and the sky
mask against the restatement (tests/track_restatement.py), the ICP schedule stage by stage against the restated chain, the tracker
end to end on motion-distorted scans, the handover of an emitted frame to the mapper, and the errors."""

import numpy as np
import pytest
import torch

from tests import track_restatement as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_ULP_OF_ONE = float(np.spacing(np.float32(1.0)))


def _frame(dirs, dist, ts, device=DEV):
    from loner_amd.common.frame import Frame
    from loner_amd.common.sensors import LidarScan
    as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).clone()
    frame = Frame(None, LidarScan(as_t(dirs), as_t(dist), as_t(ts)))
    return frame.to(device) if device is not None else frame


def _settings(downsample="UNIFORM", mocomp=True, sky=False):
    from loner_amd.common.settings import default_tracking_settings
    s = default_tracking_settings()
    s["tracker"]["icp"]["downsample"]["type"] = downsample
    s["tracker"]["motion_compensation"]["enabled"] = mocomp
    s["tracker"]["compute_sky_rays"] = sky
    return s


def _tracker(settings, device=DEV):
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    rgb, lidar, frames = Signal(), Signal(), Signal()
    tracker = Tracker(settings, rgb, lidar, frames, device=device)
    return tracker, lidar, frames.register()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---------------------------------------------------------------- 1. frame cloud
def test_frame_cloud_equals_the_reference_bit_for_bit():
    from loner_amd.analysis.lidar_map import PointCloud
    from loner_amd.utils import synthetic as SY
    g = TR.g16()
    for name in ("all", "window", "uniform", "short"):
        ts = g["timestamps_short" if name == "short" else "timestamps"]
        cloud = _frame(g["directions"], g["distances"], ts).build_point_cloud(*TR.g16_cloud_args(g, name))
        assert isinstance(cloud, PointCloud) and cloud.points.is_cuda and cloud.points.dtype == torch.float64
        assert _same_bits(cloud.numpy(), g[f"cloud_{name}"].astype(np.float64)), name
    dirs, ts = SY.lidar_pattern()
    dist = SY.scene_ranges(dirs, torch.eye(4))
    for duration, target in ((None, None), (0.9, None), (0.9, 5000), (0.5, 777)):
        a, b, s, want = TR.frame_cloud(dirs, dist, ts, duration, target)
        frame = _frame(dirs, dist, ts)
        assert frame.cloud_window(duration, target) == (a, b, s)
        assert _same_bits(frame.build_point_cloud(duration, target).numpy(), want), (duration, target)


# ---------------------------------------------------------------- 2. motion compensation
def _compensate(dirs, dist, ts, T_s, T_e, t0, t1, T_target):
    from loner_amd.common.pose import Pose
    frame = _frame(dirs, dist, ts)
    scan = frame.lidar_points
    stamps = scan.timestamps.clone()
    scan.motion_compensate((Pose(torch.as_tensor(T_s).clone()).to(DEV), Pose(torch.as_tensor(T_e).clone()).to(DEV)),
                           (torch.as_tensor(t0).to(DEV), torch.as_tensor(t1).to(DEV)), Pose(torch.as_tensor(T_target).clone()).to(DEV), True)
    assert torch.equal(scan.timestamps, stamps)                                  # timestamps are untouched
    assert scan.ray_directions.dtype == torch.float32 and scan.distances.dtype == torch.float32
    return scan.ray_directions.cpu().numpy(), scan.distances.cpu().numpy()


def test_motion_compensation_is_the_fp64_value_rounded_once():
    """distances within 1 fp32 ulp of the fp64 restatement, direction components within 1 ulp of 1, and so never further from it than
    the reference's own fp32 chain is on G16.  First measurement (G16, 4 096 rays, world coordinates to 75 m): distances 3.8e-6 m
    (0.50 ulp) and directions 3.0e-8 in all three cases, where the reference's fp32 chain is at 1.1e-5 .. 1.5e-5 m and 1.6e-7 .. 2.0e-7;
    65 536 rays to 77 m: 0.50 ulp, 3.0e-8."""
    g = TR.g16()
    for name in ("general", "same_rotation", "beyond"):
        T_s, T_e = g[f"mocomp_{name}_poses"]
        t0, t1 = g[f"mocomp_{name}_times"]
        got_dirs, got_dist = _compensate(g["directions"], g["distances"], g["timestamps"], T_s, T_e, t0, t1, T_e)
        again_dirs, again_dist = _compensate(g["directions"], g["distances"], g["timestamps"], T_s, T_e, t0, t1, T_e)
        assert np.array_equal(got_dirs.view(np.uint32), again_dirs.view(np.uint32)) and np.array_equal(got_dist.view(np.uint32), again_dist.view(np.uint32))
        e_dist, e_dir, want_dirs, want_dist = TR.g16_mocomp_errors(g, name, got_dirs, got_dist)
        ref_dist, ref_dir, _, _ = TR.g16_mocomp_errors(g, name, g[f"mocomp_{name}_directions"], g[f"mocomp_{name}_distances"])
        ulps = np.abs(got_dist.astype(np.float64) - want_dist) / np.spacing(want_dist.astype(np.float32)).astype(np.float64)
        print(f"{name}: kernel distance error {e_dist:.3g} m ({ulps.max():.2f} ulp), direction {e_dir:.3g}; "
              f"reference distance error {ref_dist:.3g} m, direction {ref_dir:.3g}")
        assert ulps.max() <= 1.0, (name, ulps.max())
        assert e_dir <= F32_ULP_OF_ONE, (name, e_dir)
        assert e_dist <= ref_dist and e_dir <= ref_dir, (name, e_dist, ref_dist, e_dir, ref_dir)
    # the cases cover the theta < 1e-9 branch and f > 1 (asserted on the fixture in tests/test_tracking_host.py); a 65 536-ray scan with
    # ranges to 78 m, compensated into a third frame
    from loner_amd.common.pose_utils import tensor_to_transform
    from loner_amd.utils import synthetic as SY
    dirs, ts = SY.lidar_pattern()
    dist = SY.scene_ranges(dirs, torch.eye(4))
    T_s, T_e, T_t = (tensor_to_transform(torch.tensor(p)).float() for p in
                     ([0.3, 0.1, 0.0, 0.01, -0.02, 0.05], [0.62, 0.13, 0.01, 0.012, -0.024, 0.09], [0.5, 0.0, 0.0, 0.0, 0.0, 0.07]))
    got_dirs, got_dist = _compensate(dirs, dist, ts, T_s, T_e, -0.01, 0.08, T_t)
    want_dirs, want_dist = TR.motion_compensate(dirs, dist, ts, T_s, T_e, torch.tensor(-0.01), torch.tensor(0.08), T_t)
    ulps = np.abs(got_dist.astype(np.float64) - want_dist) / np.spacing(want_dist.astype(np.float32)).astype(np.float64)
    print(f"65 536 rays to {float(dist.max()):.1f} m: {ulps.max():.2f} ulp, direction {np.abs(got_dirs - want_dirs).max():.3g}")
    assert ulps.max() <= 1.0 and np.abs(got_dirs - want_dirs).max() <= F32_ULP_OF_ONE


# ---------------------------------------------------------------- 3. sky rays
def test_sky_rays_match_the_restatement_in_count_order_and_value():
    """Same count, same order, components within 1e-6.  First measurement: 2 423 candidates, 1 909 kept, largest component error 1.8e-7;
    the nearest point is 3.8e-3 degrees from a half-integer, the nearest candidate 3.3e-3 degrees from the cut."""
    from loner_amd.common.pose import Pose
    dirs, R = TR.sky_case()
    want, diag = TR.sky_rays(dirs, R)
    assert diag["tie_margin_deg"] > 1e-3 and diag["cut_margin_deg"] > 1e-3, diag       # no rounding tie, no candidate on the cut
    assert (diag["candidates"], want.shape[1]) == (2423, 1909)
    T = torch.eye(4)
    T[:3, :3] = R
    frame = _frame(dirs, torch.ones(dirs.shape[1]), torch.linspace(0, 0.1, dirs.shape[1]))
    frame._lidar_pose = Pose(T).to(DEV)
    tracker, _, _ = _tracker(_settings(sky=True))
    tracker.compute_sky_rays(frame)
    got = frame.lidar_points.sky_rays
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous()
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    err = float((got.cpu() - want).abs().max())
    print(f"{diag}; {got.shape[1]} sky rays, max component error {err:.3g}")
    assert err <= 1e-6


def test_sky_mask_borders_on_a_hand_made_image():
    """The closing's border rules as a property of the kernel: directions on whole degrees fill an image of polar angles 40 .. 70 by
    360 azimuths except for hand-made holes.  A one-pixel hole and a 2x2 hole on the left edge away from the corner close; a 3x3 hole
    and the 2x2 holes in the bottom-right and bottom-left corners survive (out-of-image neighbours are ignored, columns 0 and 359 are
    not neighbours): 17 sky rays, all more than 20 degrees above the horizon, in row-major order."""
    from loner_amd.common.pose import Pose
    polar, azimuth = np.meshgrid(np.arange(40, 71), np.arange(-180, 180), indexing="ij")
    filled = np.ones(polar.shape, dtype=bool)
    filled[10, 100] = False                 # closes
    filled[12:14, 0:2] = False              # closes: the rows above and below reach it
    filled[15:18, 200:203] = False          # survives
    filled[29:31, 358:360] = False          # survives
    filled[29:31, 0:2] = False              # survives: no azimuth wrap
    p, a = np.deg2rad(polar[filled].astype(np.float64)), np.deg2rad(azimuth[filled].astype(np.float64))
    dirs = torch.tensor(np.stack([np.sin(p) * np.cos(a), np.sin(p) * np.sin(a), np.cos(p)]), dtype=torch.float32)
    yaw = np.deg2rad(3.7)
    T = torch.eye(4)
    T[:2, :2] = torch.tensor([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    want, diag = TR.sky_rays(dirs, T[:3, :3])
    assert diag["candidates"] == 17 and want.shape[1] == 17 and diag["rows"] == 31 and diag["cut_margin_deg"] > 9
    survivors = [(r, c) for r in (15, 16, 17) for c in (200, 201, 202)] + [(r, c) for r in (29, 30) for c in (0, 1, 358, 359)]
    pr, az = np.deg2rad([r + 40.0 for r, _ in sorted(survivors)]), np.deg2rad([c - 180.0 + 3.7 for _, c in sorted(survivors)])
    by_hand = np.stack([np.sin(pr) * np.cos(az), np.sin(pr) * np.sin(az), np.cos(pr)])
    assert np.abs(want.numpy() - by_hand).max() < 1e-6                          # the restatement is the hand-made answer
    frame = _frame(dirs, torch.ones(dirs.shape[1]), torch.linspace(0, 0.1, dirs.shape[1]))
    frame._lidar_pose = Pose(T).to(DEV)
    tracker, _, _ = _tracker(_settings(sky=True))
    tracker.compute_sky_rays(frame)
    got = frame.lidar_points.sky_rays.cpu()
    assert tuple(got.shape) == (3, 17)
    assert float((got - want).abs().max()) <= 1e-6 and np.abs(got.numpy() - by_hand).max() < 2e-6


# ---------------------------------------------------------------- 4. the ICP schedule
def _scans(count, beams, azimuths):
    return [TR.distorted_scan(k, beams, azimuths) for k in range(count)]


@pytest.mark.parametrize("downsample", [None, "VOXEL", "UNIFORM"])
def test_every_stage_of_the_schedule_matches_the_restatement(downsample):
    """Three 32 x 512 motion-distorted frames: the first gets the fixed identity; for the next two every stage of the default schedule
    equals the restated stage started from the same init (1e-10 in the transformation, equal fitness, RMSE to 1e-12), and the
    reference cloud, pose and time advance.  First measurement: |dT| at most 1.1e-15 over all twelve stages (None 14 744 points,
    VOXEL 13 9xx, UNIFORM 7 372); the 1.5 m stage ends at fitness 1 and RMSE 0.155 m, the 0.125 m stage at fitness 0.58 - 0.60 and RMSE
    0.073 - 0.074 m, in 4 - 10 rounds."""
    settings = _settings(downsample, mocomp=False)
    tracker, _, _ = _tracker(settings)
    schedule = settings["tracker"]["icp"]["schedule"]
    assert [s["threshold"] for s in schedule] == [1.5, 0.125] and all(s["max_iterations"] == 10 for s in schedule)
    scans = _scans(3, 32, 512)
    prev_cloud = None
    pose = torch.eye(4)
    for k, (dirs, dist, ts) in enumerate(scans):
        frame = _frame(dirs, dist, ts)
        cloud = tracker.frame_cloud(frame).numpy()
        assert tracker.track_frame(frame)
        got_pose = frame.get_lidar_pose().get_transformation_matrix().detach().cpu()
        if k == 0:
            assert torch.equal(got_pose, torch.eye(4)) and not frame.get_lidar_pose().get_pose_tensor().requires_grad
            assert tracker.last_registrations == []
        else:
            normals = TR.normals(prev_cloud)
            init = np.eye(4)
            assert len(tracker.last_registrations) == len(schedule)
            for stage, got in zip(schedule, tracker.last_registrations):
                want = TR.icp_stage(cloud, prev_cloud, normals, stage, init)
                dT = float(np.abs(got.transformation - want["transformation"]).max())
                print(f"{downsample} frame {k} stage {stage['threshold']}: {len(cloud)} -> {len(prev_cloud)} points, |dT| {dT:.3g}, "
                      f"fitness {got.fitness:.6f}, rmse {got.inlier_rmse:.6g}, {got.iterations} rounds")
                assert dT < 1e-10, (k, stage["threshold"], dT)
                assert got.fitness == want["fitness"] and abs(got.inlier_rmse - want["inlier_rmse"]) < 1e-12
                init = got.transformation.copy()                                   # the next stage starts from this one
            pose = pose @ torch.from_numpy(init).float()
            assert float((got_pose - pose).abs().max()) < 1e-6                     # through the 6-vector of the frame's Pose
            assert torch.equal(tracker._reference_pose.get_transformation_matrix().cpu(), pose)
        assert _same_bits(tracker._reference_point_cloud.numpy(), cloud) and tracker._reference_point_cloud.has_normals()
        assert float(tracker._reference_time) == float(ts[0] / 2. + ts[-1] / 2.)
        assert _same_bits(frame.lidar_points.distances.cpu().double().numpy(), dist.double().numpy())      # compensation is off here
        prev_cloud = cloud


# ---------------------------------------------------------------- 5. end to end
def _run(scans, mocomp, sky=False):
    """the scans through Signal -> Tracker.update() -> the emitted frames"""
    tracker, lidar, out = _tracker(_settings("UNIFORM", mocomp=mocomp, sky=sky))
    frames = []
    for dirs, dist, ts in scans:
        lidar.emit((_frame(dirs, dist, ts, device=None).lidar_points, None))           # host scans: the tracker places them
        tracker.update()
        while out.has_value():
            frames.append(out.get_value())
    return tracker, frames


def _residual(frames, T_world_of_origin, poses=None):
    """mean distance of the frames' world points to the analytic surfaces; the tracker's world is the first frame's pose"""
    total, count = 0.0, 0
    for k, frame in enumerate(frames):
        scan = frame.lidar_points
        p = (scan.ray_directions * scan.distances).double().cpu().numpy()
        T = frame.get_lidar_pose().get_transformation_matrix().detach().double().cpu().numpy() if poses is None else poses[k]
        world = T_world_of_origin @ T
        d = TR.surface_distance((world[:3, :3] @ p).T + world[:3, 3])
        total, count = total + d.sum(), count + d.size
    return total / count


def test_tracker_end_to_end_on_motion_distorted_scans():
    """Ten motion-distorted 64 x 1024 frames (3 m/s, 20 deg/s) through the signals.  The poses equal the restated chain to 1e-6 in
    translation (the fp32 pose composition); the emitted scans lie closer to the analytic surfaces with motion compensation than
    without, and no closer than when compensated with the true poses.
    First measurement: poses against the restated chain 0 m in translation (1.2e-7 in the rotation entries, the 6-vector round trip);
    trajectory error against truth 0.19 m after ten frames (frame-to-frame ICP on skewed clouds, as the reference tracks); mean surface
    distance 0.0628 m compensated, 0.0779 m uncompensated, 0.0042 m when compensated with the true poses.  No threshold is set on these."""
    from loner_amd.common.pose import Pose
    scans = _scans(10, 64, 1024)
    tracker, frames = _run(scans, mocomp=True)
    _, frames_off = _run(scans, mocomp=False)
    assert len(frames) == len(frames_off) == 10 and [f._id for f in frames] == list(range(10))
    # the restated chain on the clouds the tracker saw
    clouds = [TR.frame_cloud(d, r, t, 0.9, 5000)[3] for d, r, t in scans]
    want, _ = TR.track_chain(clouds, _settings()["tracker"]["icp"]["schedule"])
    got = torch.stack([f.get_lidar_pose().get_transformation_matrix().detach().cpu() for f in frames])
    got_off = torch.stack([f.get_lidar_pose().get_transformation_matrix().detach().cpu() for f in frames_off])
    assert torch.equal(got, got_off)                                            # compensation does not feed back into tracking
    err = float((got[:, :3, 3] - want[:, :3, 3]).abs().max())
    print(f"poses against the restated chain: translation {err:.3g} m, rotation entries {float((got[:, :3, :3] - want[:, :3, :3]).abs().max()):.3g}")
    assert err <= 1e-6
    # against the truth: the pose of frame k at its middle time, relative to frame 0's
    mid = [float(t[0] / 2. + t[-1] / 2.) for _, _, t in scans]
    truth = TR.pose_at(np.array(mid))
    origin = truth[0]
    rel_truth = np.linalg.inv(origin) @ truth
    traj = np.abs(got[:, :3, 3].double().numpy() - rel_truth[:, :3, 3]).max()
    on, off = _residual(frames, origin), _residual(frames_off, origin)
    # the same scans compensated with the true poses of consecutive middle times, mapped with the true pose
    true_frames = []
    for k, (dirs, dist, ts) in enumerate(scans):
        frame = _frame(dirs, dist, ts)
        if k:
            P = lambda T: Pose(torch.from_numpy(T).float()).to(DEV)
            frame.lidar_points.motion_compensate((P(rel_truth[k - 1]), P(rel_truth[k])), (torch.tensor(mid[k - 1]), torch.tensor(mid[k])),
                                                 P(rel_truth[k]), True)
        true_frames.append(frame)
    best = _residual(true_frames, origin, poses=[T.astype(np.float32).astype(np.float64) for T in rel_truth])
    print(f"trajectory error against truth {traj:.4g} m; mean surface distance: compensated {on:.4g} m, uncompensated {off:.4g} m, "
          f"compensated with the true poses {best:.4g} m")
    assert on < off and on >= best


# ---------------------------------------------------------------- 6. handover to the mapper
def test_an_emitted_frame_goes_into_the_mapper():
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.mapping.keyframe import KeyFrame
    from loner_amd.mapping.optimizer import Optimizer
    from loner_amd.utils import synthetic as SY
    from tests.support import small_settings
    scans = [TR.open_sky(*scan) for scan in _scans(2, 64, 1024)]          # every ray of the closed scene returns: open a patch of sky
    _, frames = _run(scans, mocomp=True, sky=True)
    frame = frames[1]
    sky = frame.lidar_points.sky_rays
    assert sky is not None and sky.shape[0] == 3 and sky.shape[1] > 64
    s = small_settings(64, 64)
    s["num_samples"]["sky"] = 16
    s["keyframe_schedule"] = [{"num_keyframes": -1, "iteration_schedule": [
        {"num_iterations": 6, "freeze_poses": True, "freeze_sigma_mlp": False, "freeze_rgb_mlp": True}]}]
    scale, shift = SY.world_cube()
    wc = WorldCube(torch.tensor(scale), torch.from_numpy(shift))
    torch.manual_seed(0)
    opt = Optimizer(s, None, wc, 0, False, True, True)
    kf = KeyFrame(frame, 0)
    rays, depths = kf.build_lidar_rays(torch.arange(8, device=DEV), torch.tensor([1.0, 50.0]), wc.to(DEV, clone=True),
                                       sky_indices=torch.arange(4, device=DEV))
    # the sky scan goes through the pose like any scan (keyframe.py:91-100): its rays are the stored directions turned by the pose
    R = frame.get_lidar_pose().get_rotation().detach().to(rays.device)
    assert rays.shape == (12, 13) and torch.allclose(rays[8:, 3:6], (R @ sky[:, :4].to(rays.device)).T, atol=1e-5)
    opt.iterate_optimizer([kf])
    assert opt.last_stats["n_valid_rays"] == 6 * (64 + 16) and torch.isfinite(opt.last_stats["loss_terms"]).all()


# ---------------------------------------------------------------- 7. errors
def test_errors():
    from loner_amd.common.pose import Pose
    from loner_amd.common.sensors import LidarScan
    from loner_amd.common.frame import Frame
    dirs, dist, ts = TR.distorted_scan(0, 8, 64)
    tracker, _, _ = _tracker(_settings(), device=None)
    with pytest.raises(RuntimeError):                         # a scan on the CPU
        tracker.track_frame(_frame(dirs, dist, ts, device=None))
    with pytest.raises(RuntimeError):
        _frame(dirs, dist, ts, device=None).build_point_cloud(0.9)
    with pytest.raises(ValueError):                           # an empty scan
        tracker.track_frame(Frame(None, LidarScan()))
    with pytest.raises(ValueError):
        Frame(None, LidarScan()).build_point_cloud()
    with pytest.raises(ValueError):                           # an unknown downsample type
        _tracker(_settings("RANDOM"))
    with pytest.raises(NotImplementedError):                  # the debug dumps
        s = _settings()
        s["tracker"]["debug"]["write_icp_point_clouds"] = True
        _tracker(s)
    bad = torch.eye(4)
    bad[0, 3] = float("nan")
    frame = _frame(dirs, dist, ts)
    before = frame.lidar_points.distances.clone()
    with pytest.raises(ValueError):                           # a non-finite pose
        frame.lidar_points.motion_compensate((Pose(torch.eye(4)).to(DEV), Pose(bad.clone()).to(DEV)), (0.0, 0.1), Pose(torch.eye(4)).to(DEV))
    assert torch.equal(frame.lidar_points.distances, before)
    bad_rotation = torch.eye(4)
    bad_rotation[1, 1] = float("inf")
    frame._lidar_pose = Pose(bad_rotation).to(DEV)
    with pytest.raises(ValueError):
        tracker.compute_sky_rays(frame)
    nan_dirs = dirs.clone()
    nan_dirs[1, 5] = float("nan")
    frame = _frame(nan_dirs, dist, ts)
    frame._lidar_pose = Pose(torch.eye(4)).to(DEV)
    with pytest.raises(RuntimeError):                         # a non-finite direction sets no pixel and is reported
        tracker.compute_sky_rays(frame)
