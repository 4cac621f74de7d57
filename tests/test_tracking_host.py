"""The tracker's host side on the CPU: the restatement (tests/track_restatement.py) against the reference's recorded outputs
(tests/golden/g16_tracking.npz), FrameSynthesis's accept sequences, hand-made known answers for the sky mask's closing, and pickling."""
import pickle

import numpy as np
import torch

from tests import track_restatement as TR

def test_frame_cloud_restatement_equals_the_reference_bit_for_bit():
    g = TR.g16()
    dirs, dist = torch.from_numpy(g["directions"]), torch.from_numpy(g["distances"])
    sizes = {}
    for name in ("all", "window", "uniform", "short"):
        ts = torch.from_numpy(g["timestamps_short" if name == "short" else "timestamps"])
        a, b, s, pts = TR.frame_cloud(dirs, dist, ts, *TR.g16_cloud_args(g, name))
        want = g[f"cloud_{name}"].astype(np.float64)
        assert pts.shape == want.shape, (name, pts.shape, want.shape)
        assert np.array_equal(pts.view(np.uint64), want.view(np.uint64)), name
        sizes[name] = (a, b, s, len(pts))
    n = dirs.shape[1]
    assert sizes["all"] == (0, n, 1, n) and sizes["short"][:2] == (0, n) and sizes["short"][2] == n // 500
    assert 0 < sizes["window"][0] < sizes["window"][1] < n and sizes["uniform"][2] == (sizes["window"][1] - sizes["window"][0]) // 500


def test_motion_compensation_restatement_agrees_with_the_reference():
    """The reference's chain is about ten fp32 roundings on world-frame magnitudes: within 16 fp32 ulps of the largest world-frame
    coordinate for distances, 16 ulps of 1 for direction components."""
    g = TR.g16()
    ulp = float(np.spacing(np.float32(TR.g16_world_magnitude(g))))
    for name in ("general", "same_rotation", "beyond"):
        e_dist, e_dir, _, _ = TR.g16_mocomp_errors(g, name, g[f"mocomp_{name}_directions"], g[f"mocomp_{name}_distances"])
        print(f"{name}: distance error {e_dist:.3g} m ({e_dist / ulp:.2f} ulp of {TR.g16_world_magnitude(g):.1f} m), direction error {e_dir:.3g}")
        assert e_dist <= 16 * ulp, (name, e_dist, ulp)
        assert e_dir <= 16 * float(np.spacing(np.float32(1.0))), (name, e_dir)
    # the cases are what they claim to be: an identical-rotation pair, and factors beyond 1
    same = g["mocomp_same_rotation_poses"]
    assert np.array_equal(same[0][:3, :3], same[1][:3, :3]) and not np.array_equal(same[0][:3, 3], same[1][:3, 3])
    t0, t1 = g["mocomp_beyond_times"]
    assert float(((g["timestamps"] - t0) / (t1 - t0)).min()) > 1.0


def _synthesis_settings(decimate):
    from loner_amd.common.settings import default_tracker_settings
    s = default_tracker_settings().frame_synthesis
    s["decimate_on_load"] = decimate
    return s


def test_frame_synthesis_accepts_what_the_reference_accepts():
    from loner_amd.common.pose import Pose
    from loner_amd.common.sensors import LidarScan
    from loner_amd.tracking.frame_synthesis import FrameSynthesis
    g = TR.g16()
    for decimate in (True, False):
        synth = FrameSynthesis(_synthesis_settings(decimate), Pose(), True)
        accepted = []
        for k, t in enumerate(g["synthesis_times"]):
            stamps = torch.tensor([t, t + 0.01, t + 0.02, t + 0.03], dtype=torch.float32)
            synth.process_lidar(LidarScan(torch.zeros(3, 4), torch.ones(4), stamps), None)
            while synth.has_frame():
                frame = synth.pop_frame()
                assert len(frame.lidar_points) == 4 and frame.lidar_points.timestamps is not stamps          # a clone
                accepted.append(k)
        assert accepted == g[f"synthesis_accepted_decimate_{int(decimate)}"].tolist(), decimate
    assert len(g["synthesis_accepted_decimate_0"]) < len(g["synthesis_accepted_decimate_1"]) == len(g["synthesis_times"])


def test_frame_synthesis_matches_images_to_scans():
    """the image path (frame_synthesis.py:75-126): an image takes the first scan whose widened time range holds it and drops the
    scans before it; images closer than a frame period are decimated"""
    from types import SimpleNamespace
    from loner_amd.common.pose import Pose
    from loner_amd.common.sensors import LidarScan
    from loner_amd.tracking.frame_synthesis import FrameSynthesis

    class Image(SimpleNamespace):
        def clone(self):
            return Image(image=self.image.clone(), timestamp=self.timestamp)

    synth = FrameSynthesis(_synthesis_settings(True), Pose(), False)
    for k in range(4):
        t = 0.1 * k
        synth.process_lidar(LidarScan(torch.zeros(3, 2), torch.full((2,), float(k)), torch.tensor([t, t + 0.09])), None)
    assert not synth.has_frame()
    synth.process_image(Image(image=torch.zeros(1), timestamp=0.15))
    synth.process_image(Image(image=torch.zeros(1), timestamp=0.2))          # 0.05 s later: decimated
    synth.process_image(Image(image=torch.zeros(1), timestamp=0.35))
    first, second = synth.pop_frame(), synth.pop_frame()
    assert float(first.lidar_points.distances[0]) == 1.0 and float(second.lidar_points.distances[0]) == 3.0
    assert not synth.has_frame() and synth.pop_frame() is None and len(synth._lidar_scans) == 0


def _closed(img):
    return TR.closing(torch.tensor(img, dtype=torch.float32)).numpy()


def test_sky_mask_closing_known_answers():
    ones = np.ones((12, 360), dtype=np.float32)
    hole1 = ones.copy()
    hole1[6, 100] = 0                                    # a one-pixel hole closes
    assert _closed(hole1).min() == 1
    hole3 = ones.copy()
    hole3[6:9, 100:103] = 0                              # a 3x3 hole: its centre survives the dilation, the erosion restores it
    want = ones.copy()
    want[6:9, 100:103] = 0
    assert np.array_equal(_closed(hole3), want)
    corner = ones.copy()
    corner[10:12, 358:360] = 0                           # a 2x2 hole in the image corner survives: out-of-image neighbours are ignored
    want = ones.copy()
    want[10:12, 358:360] = 0
    assert np.array_equal(_closed(corner), want)
    left = ones.copy()
    left[10:12, 0:2] = 0                                 # the same at column 0: columns 0 and 359 are not neighbours (with an azimuth
    want = ones.copy()                                   # wrap, the set pixels of column 359 would close it)
    want[10:12, 0:2] = 0
    assert np.array_equal(_closed(left), want)
    edge = ones.copy()
    edge[6:8, 0:2] = 0                                   # away from the corner the rows above and below close it
    assert _closed(edge).min() == 1
    empty = np.zeros((8, 360), dtype=np.float32)
    out = _closed(empty)                                 # the top three rows are set, nothing else
    assert out[:3].min() == 1 and out[3:].max() == 0


def test_sky_image_folds_column_360_and_offsets_by_the_minima():
    deg = np.deg2rad
    az = np.array([-179.6, 179.7, -90.0, 0.0, 179.0])      # -180, +180, ...: +180 lands in column 360
    el = np.array([80.0, 85.0, 90.0, 95.0, 100.0])         # the polar angle phi
    d = torch.tensor(np.stack([np.sin(deg(el)) * np.cos(deg(az)), np.sin(deg(el)) * np.sin(deg(az)), np.cos(deg(el))]), dtype=torch.float32)
    theta, phi = TR.integer_degrees(d)
    assert phi.tolist() == [80, 85, 90, 95, 100] and theta.tolist() == [-180, 180, -90, 0, 179]
    img, polar_min, azimuth_min = TR.sky_image(d)
    assert (polar_min, azimuth_min) == (80, -180)
    assert img.shape == (21, 360) and int(img.sum()) == 5
    assert img[0, 0] == 1 and img[5, 0] == 1 and img[10, 90] == 1 and img[15, 180] == 1 and img[20, 359] == 1


def test_sky_rays_restatement_on_the_test_pattern():
    """the GPU test's input (tests/test_gpu_tracking.py): no rounding tie within 1e-3 degrees, no candidate within 1e-3 degrees of
    the cut, the candidate and kept counts the test was designed with"""
    dirs, R = TR.sky_case()
    rays, diag = TR.sky_rays(dirs, R)
    print(diag, rays.shape)
    assert diag["tie_margin_deg"] > 1e-3 and diag["cut_margin_deg"] > 1e-3
    assert (diag["candidates"], rays.shape[1]) == (2423, 1909)
    assert float((rays.norm(dim=0) - 1).abs().max()) < 1e-6


def test_tracker_and_settings_pickle_before_first_use():
    from loner_amd.common.settings import default_tracker_settings, default_tracking_settings
    from loner_amd.common.signals import Signal, StopSignal
    from loner_amd.tracking.tracker import Tracker
    s = default_tracker_settings()
    back = pickle.loads(pickle.dumps(s))
    assert back == s and back.icp.schedule[1].threshold == 0.125 and back.icp.downsample.type == "UNIFORM"
    assert back.frame_synthesis.frame_decimation_rate_hz == 5 and back.icp.scan_duration == 0.9 and back.compute_sky_rays is False
    rgb, lidar, frames = Signal(), Signal(), Signal()
    tracker = Tracker(default_tracking_settings(), rgb, lidar, frames)
    clone = pickle.loads(pickle.dumps(tracker))
    assert clone._reference_point_cloud is None and clone._frame_count == 0
    # the signals: every slot gets its own copy, first in first out; a stop signal ends the tracker
    slot_a, slot_b = frames.register(), frames.register()
    value = [1, 2]
    frames.emit(value)
    frames.emit("second")
    assert slot_a.has_value() and slot_a.get_value() == [1, 2] and slot_a.get_value() == "second" and slot_a.get_value() is None
    assert slot_b.get_value() is not value and len(slot_b) == 1
    frames.flush()
    assert not slot_b.has_value()
    lidar.emit(StopSignal())
    tracker.update()
    assert tracker._processed_stop_signal


def test_scan_and_frame_members():
    from loner_amd.common.frame import Frame
    from loner_amd.common.pose import Pose
    from loner_amd.common.sensors import LidarScan
    a = LidarScan(torch.zeros(3, 4), torch.ones(4), torch.arange(4.0))
    b = LidarScan(torch.ones(3, 2), torch.full((2,), 2.0), torch.tensor([4.0, 5.0]), sky_rays=torch.ones(3, 1))
    a.merge(b)
    assert len(a) == 6 and a.ray_directions.shape == (3, 6) and a.sky_rays.shape == (3, 1)
    a.remove_points(4)
    assert a.distances.tolist() == [2.0, 2.0] and a.timestamps.tolist() == [4.0, 5.0]
    frame = Frame(None, a)
    frame._lidar_pose = Pose(torch.eye(4))
    copy = frame.clone()
    assert copy.lidar_points is not a and torch.equal(copy.lidar_points.timestamps, a.timestamps) and copy._gt_lidar_pose is None
    assert float(frame.get_middle_time()) == 4.5 and frame.get_scan_duration() == 1.0 and frame.detach() is frame
    assert len(a.clear()) == 0 and a.sky_rays.numel() == 0
    empty = LidarScan().add_points(torch.zeros(3, 1), torch.ones(1), torch.zeros(1))
    assert len(empty) == 1
    # calibration entries: None is the identity; a quarter turn about z
    assert torch.equal(Pose.from_settings(None).get_transformation_matrix(), torch.eye(4))
    q = Pose.from_settings({"xyz": [1.0, 2.0, 3.0], "orientation": [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]})
    want = torch.tensor([[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    assert torch.allclose(q.get_transformation_matrix(), want, atol=1e-6)
