"""LiDAR SLAM end to end on the MI355X (loner_amd.loner.Loner): twelve motion-distorted 32 x 512 scans handed in as raw (xyz, t)
arrays through build_scan_from_points, tracked, mapped on four keyframes and logged.  The log directory's layout, the loop adding
nothing to tracking, frozen poses, run-to-run determinism, and the package's own consumers reading final.tar.

Keyframes are TEMPORAL, every third frame.  The stamps are fp32 (0.9f - 0.6f = 0.29999995 < 0.3), so the threshold is set to 0.29 s:
frames 0, 3, 6 and 9 become keyframes whichever way the stamps round."""
import os

import numpy as np
import pytest
import torch

from tests import slam_restatement as SR
from tests import track_restatement as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
FRAMES, BEAMS, AZIMUTHS, PERIOD = 12, 32, 512, 0.1
KEYFRAME_FRAMES = [0, 3, 6, 9]
FIRST_ITERATIONS, LATER_ITERATIONS = 60, 20
TRAJECTORIES = ("tracking_only", "online_estimates", "keyframe_trajectory", "estimated_trajectory")
FULL_KEYS = {"global_step", "network_state_dict", "optimizer_state_dict", "poses", "occ_model_state_dict", "occ_optimizer_state_dict"}

_raw = []


def raw_scans():
    """[(xyz [n,3] fp32, local times [n] fp64, stamp, ground-truth pose fp32 [4,4])] of the twelve scans, built once"""
    if not _raw:
        for k in range(FRAMES):
            dirs, dist, ts = TR.distorted_scan(k, BEAMS, AZIMUTHS, PERIOD)
            local = ts.double() - k * PERIOD
            _raw.append(((dirs * dist).T.contiguous(), local, k * PERIOD, torch.from_numpy(TR.pose_at(k * PERIOD)[0]).float()))
    return _raw


def ingested(k):
    from loner_amd.common.sensors import build_scan_from_points
    xyz, local, stamp, _ = raw_scans()[k]
    return build_scan_from_points(xyz, local, stamp, device=DEV)[0]


def slam_settings(log_dir_prefix, freeze_poses=False):
    from loner_amd.common.settings import default_settings
    from tests.support import small_settings
    s = default_settings(str(log_dir_prefix), (1, 50))
    optimizer = dict(small_settings(256, 64))
    for key in ("debug", "log_directory"):
        optimizer.pop(key)
    optimizer["freeze_poses"] = freeze_poses
    optimizer["keyframe_schedule"] = [
        {"num_keyframes": 1, "iteration_schedule": [
            {"num_iterations": FIRST_ITERATIONS, "freeze_poses": True, "freeze_sigma_mlp": False, "freeze_rgb_mlp": True}]},
        {"num_keyframes": -1, "iteration_schedule": [
            {"num_iterations": LATER_ITERATIONS, "freeze_poses": False, "freeze_sigma_mlp": False, "freeze_rgb_mlp": True}]}]
    s["mapper"]["optimizer"] = optimizer
    s["mapper"]["log_level"] = "VERBOSE"
    s["mapper"]["keyframe_manager"]["keyframe_selection"].update(strategy="TEMPORAL", temporal={"time_diff_seconds": 0.29})
    s["system"]["single_threaded"] = True
    s["tracker"]["frame_synthesis"].update(frame_decimation_rate_hz=10, decimate_on_load=False)     # 0.1 s apart: every frame is due
    s["debug"]["flags"]["log_times"] = True
    return s


def run_slam(log_dir_prefix, name, seed=0, freeze_poses=False):
    from loner_amd.common.pose import Pose
    from loner_amd.loner import Loner
    torch.manual_seed(seed)
    loner = Loner(slam_settings(log_dir_prefix, freeze_poses))
    truth = torch.stack([r[3] for r in raw_scans()])
    loner.initialize(None, truth, None, [1, 50], None, str(log_dir_prefix), experiment_name=name)
    loner.start()
    for k in range(FRAMES):
        loner.process_lidar(ingested(k), Pose(truth[k].clone()))
    loner.stop()
    return loner


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the run every test reads, a second one from the same seed, and one with the poses frozen"""
    root = tmp_path_factory.mktemp("slam")
    return {name: run_slam(root, name, freeze_poses=(name == "frozen")) for name in ("first", "again", "frozen")}


def _trajectory(loner, name):
    from loner_amd.common.pose_utils import read_tum
    return read_tum(os.path.join(loner.get_log_directory(), "trajectory", name + ".txt"))


def _text(loner, *parts):
    return open(os.path.join(loner.get_log_directory(), *parts)).read()


def test_the_log_directory_has_the_layout_the_analysis_tools_read(runs):
    loner = runs["first"]
    log = loner.get_log_directory()
    assert log.endswith("/first/")
    names = [f"ckpt_{k}" for k in range(4)] + ["final"]
    assert sorted(os.listdir(os.path.join(log, "checkpoints"))) == sorted(n + ".tar" for n in names)
    stamps = _trajectory(loner, "tracking_only")[:, 0]
    for k, name in enumerate(names):
        ckpt = torch.load(os.path.join(log, "checkpoints", name + ".tar"), map_location="cpu", weights_only=False)
        assert set(ckpt) == FULL_KEYS, name
        count = min(k + 1, 4)
        assert len(ckpt["poses"]) == count
        assert [float(p["timestamp"]) for p in ckpt["poses"]] == [float(np.float32(stamps[f])) for f in KEYFRAME_FRAMES[:count]]
        assert ckpt["global_step"] == FIRST_ITERATIONS + LATER_ITERATIONS * (count - 1)
    for name in ("world_cube.yaml", "full_config.yaml", "full_config.pkl", "map_times.csv", "track_times.csv"):
        assert os.path.getsize(os.path.join(log, name)) > 0, name
    assert [len(_trajectory(loner, name)) for name in TRAJECTORIES] == [12, 12, 4, 12]
    assert np.array_equal(_trajectory(loner, "keyframe_trajectory")[:, 0], stamps[KEYFRAME_FRAMES])
    assert np.abs(stamps - PERIOD * np.arange(FRAMES)).max() < 1e-6
    opt = loner._mapper._optimizer
    assert opt._keyframe_count == 4 and opt._global_step == FIRST_ITERATIONS + 3 * LATER_ITERATIONS
    assert len(_text(loner, "map_times.csv").split()) == 4 and len(_text(loner, "track_times.csv").split()) == 12


def test_the_loop_adds_nothing_to_tracking(runs, tmp_path):
    """tracking_only equals, bit for bit, what a bare Tracker emits for the same scans"""
    from loner_amd.common.pose_utils import dump_trajectory_to_tum
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    s = slam_settings(tmp_path)
    s["tracker"]["debug"] = {k: False for k in s["debug"]["flags"]}
    s["tracker"]["log_directory"] = str(tmp_path)
    rgb, lidar, frames = Signal(), Signal(), Signal()
    out = frames.register()
    tracker = Tracker(s, rgb, lidar, frames, device=torch.device(DEV, 0))
    poses, stamps = [], []
    for k in range(FRAMES):
        lidar.emit((ingested(k), None))
        tracker.update()
        frame = out.get_value()
        poses.append(frame.get_lidar_pose().get_transformation_matrix().detach().cpu())
        stamps.append(torch.as_tensor(frame.get_time()).detach().cpu().reshape(1).float())
    assert not out.has_value()
    dump_trajectory_to_tum(torch.stack(poses), torch.cat(stamps), str(tmp_path / "bare.txt"))
    assert open(tmp_path / "bare.txt").read() == _text(runs["first"], "trajectory", "tracking_only.txt")


def test_with_frozen_poses_the_estimate_is_the_tracking(runs):
    """nothing moves a keyframe, so every frame hung off its keyframe lands where the tracker put it: 1e-5 m covers the fp32
    products kf @ inv(tracked_kf) @ tracked at a few metres from the origin"""
    loner = runs["frozen"]
    estimated, tracked, keyframes = (_trajectory(loner, n) for n in ("estimated_trajectory", "tracking_only", "keyframe_trajectory"))
    assert np.abs(estimated[:, 1:4] - tracked[:, 1:4]).max() <= 1e-5
    assert np.array_equal(estimated[KEYFRAME_FRAMES, 0], keyframes[:, 0])
    assert np.abs(estimated[KEYFRAME_FRAMES, 1:] - keyframes[:, 1:]).max() <= 1e-5
    # and with the poses free the optimiser did move them
    free = _trajectory(runs["first"], "keyframe_trajectory")
    print(f"free poses: keyframes moved by up to {np.abs(free[:, 1:4] - keyframes[:, 1:4]).max():.3g} m")


def test_two_runs_from_the_same_seed_are_bit_identical(runs):
    a, b = runs["first"], runs["again"]
    load = lambda loner: torch.load(os.path.join(loner.get_log_directory(), "checkpoints", "final.tar"), map_location="cpu", weights_only=False)
    ca, cb = load(a), load(b)
    assert set(ca["network_state_dict"]) == set(cb["network_state_dict"])
    for key, value in ca["network_state_dict"].items():
        assert torch.equal(value, cb["network_state_dict"][key]), key
    assert torch.equal(ca["occ_model_state_dict"]["occupancy_grid"], cb["occ_model_state_dict"]["occupancy_grid"])
    for name in TRAJECTORIES:
        assert _text(a, "trajectory", name + ".txt") == _text(b, "trajectory", name + ".txt"), name


def test_final_tar_feeds_the_consumers_and_the_trajectories_score(runs):
    """compute_l1_depth on the last scan, LidarMapRenderer.render_map on the last keyframe, and ape of both trajectories against the
    truth at the frames' middle times.  The numbers are printed; nobody has measured this run, so no accuracy threshold is set."""
    from loner_amd.analysis.l1_depth import compute_l1_depth
    from loner_amd.analysis.lidar_map import LidarMapRenderer
    from loner_amd.analysis.trajectory import ape
    from loner_amd.common.pose import Pose
    from loner_amd.common.pose_utils import build_poses_from_df
    from loner_amd.common.ray_utils import LidarRayDirections
    from loner_amd.models.model_tcnn import Model, OccupancyGridModel
    from loner_amd.models.ray_sampling import OccGridRaySampler
    loner = runs["first"]
    ckpt = torch.load(os.path.join(loner.get_log_directory(), "checkpoints", "final.tar"), map_location="cpu", weights_only=False)
    mc = loner._settings.mapper.optimizer.model_config.model
    model = Model(mc).to(DEV)
    occ = OccupancyGridModel(mc.occ_model).to(DEV)
    model.load_state_dict(ckpt["network_state_dict"])
    occ.load_state_dict(ckpt["occ_model_state_dict"])
    sampler = OccGridRaySampler()
    sampler.update_occ_grid(occ().detach())
    model.cfg.render["N_samples_test"] = 256
    cube = loner.get_world_cube().to(DEV, clone=True)
    ray_range = torch.tensor([1.0, 50.0])
    estimated = _trajectory(loner, "estimated_trajectory")
    last_pose = Pose(build_poses_from_df(estimated[-1:])[0][0]).to(DEV)
    torch.manual_seed(5)
    l1 = compute_l1_depth(last_pose, LidarRayDirections(ingested(FRAMES - 1), chunk_size=1024), model, sampler, cube, ray_range, DEV, max_rays=1024)
    assert np.isfinite(l1)
    cloud = LidarMapRenderer(model, ckpt, cube, ray_range, resolution=2.0).render_map(DEV, sampler, 0.1, var_threshold=1e9, only_last_frame=True)
    points = cloud.numpy()
    assert len(points) > 0 and np.isfinite(points).all()
    # the truth: the sensor's pose at each frame's middle time, relative to the first
    tracked = _trajectory(loner, "tracking_only")
    middle = tracked[:, 0] + PERIOD * (BEAMS * AZIMUTHS - 1) / (BEAMS * AZIMUTHS) / 2
    truth = TR.pose_at(middle)
    truth = np.linalg.inv(truth[0]) @ truth
    gt_rows = SR.tum_rows(tracked[:, 0], truth)
    scores = {name: ape(_trajectory(loner, name), gt_rows) for name in ("estimated_trajectory", "tracking_only")}
    print(f"L1 depth on the last scan {l1:.4g} m; {len(points)} map points from the last keyframe; APE rmse (aligned): estimated "
          f"{scores['estimated_trajectory']['rmse']:.4g} m, tracking only {scores['tracking_only']['rmse']:.4g} m")
    for score in scores.values():
        assert score["pairs"] == FRAMES and np.isfinite(score["rmse"]) and np.isfinite(score["rotation_deg"]["rmse"])
