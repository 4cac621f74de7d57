#!/usr/bin/env python3
"""Sixth batch of golden fixtures, produced by IMPORTING THE REFERENCE in the build container.

    python tests/golden/make_golden6.py

G16  The tracker's host-side pieces on a 4 096-ray scan (16 beams x 256 azimuths of the synthetic scene):
       * Frame.build_point_cloud (src/common/frame.py:104-145) for (scan_duration, target_points) = (None, None), (0.9, None),
         (0.9, 500), and (0.9, 500) on a scan shorter than 1e-3 s: the slice bounds and the array handed to open3d;
       * LidarScan.motion_compensate (src/common/sensors.py:176-232) for a general pose pair, a pair with identical rotations (the
         NUMERIC_TOLERANCE branch) and timestamps beyond the end pose's time (extrapolation);
       * the accept sequence of FrameSynthesis.process_lidar (src/tracking/frame_synthesis.py:58-66) over a list of scan start
         times, with decimate_on_load on and off.
     Tracker.compute_sky_rays is not captured: kornia is not installed (tests/track_restatement.py is its definition here).

The stand-ins of make_golden.py apply for the import to succeed, plus two it lacks: pytorch3d.transforms.matrix_to_axis_angle (the
package's own restatement) and o3d.utility.Vector3dVector as the identity, so that build_point_cloud hands back its array.
Everything executing below is the reference's own code.  The fixture is data; nothing reads the reference at test time.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG                      # noqa: E402  (stubs, save)
from loner_amd.common import pose_utils as PU   # noqa: E402
from loner_amd.utils import synthetic as SY   # noqa: E402

SYNTHESIS_TIMES = [0.0, 0.05, 0.1, 0.18, 0.2, 0.35, 0.39, 0.41, 0.6, 0.78, 0.8, 1.0, 1.17, 1.19]


def main():
    MG.install_stubs()
    sys.modules["pytorch3d.transforms"].matrix_to_axis_angle = PU.matrix_to_axis_angle
    sys.modules["open3d"].utility.Vector3dVector = lambda a: a
    from common.frame import Frame
    from common.pose import Pose
    from common.sensors import LidarScan
    from tracking.frame_synthesis import FrameSynthesis

    torch.set_num_threads(8)
    dirs, _ = SY.lidar_pattern(16, 256)
    n = dirs.shape[1]
    ranges = SY.scene_ranges(dirs, PU.tensor_to_transform(SY.trajectory_pose6(8)[3]))
    ts = torch.linspace(0.3, 0.4, n)
    ts_short = torch.linspace(0.3, 0.3004, n)
    out = {"directions": dirs, "distances": ranges, "timestamps": ts, "timestamps_short": ts_short}

    # ---- Frame.build_point_cloud
    cases = {"all": (ts, None, None), "window": (ts, 0.9, None), "uniform": (ts, 0.9, 500), "short": (ts_short, 0.9, 500)}
    for name, (stamps, duration, target) in cases.items():
        frame = Frame(None, LidarScan(dirs.clone(), ranges.clone(), stamps.clone()))
        pts = np.asarray(frame.build_point_cloud(duration, target).points)
        assert pts.dtype == np.float32 or np.array_equal(pts, pts.astype(np.float32))
        out[f"cloud_{name}"] = pts.astype(np.float32)          # every coordinate is an fp32 product: stored without loss
        out[f"cloud_{name}_args"] = np.array([np.nan if duration is None else duration, -1 if target is None else target])

    # ---- LidarScan.motion_compensate
    p_a = torch.tensor([0.9, -0.1, 0.02, 0.004, -0.003, 0.06])
    p_b = torch.tensor([1.2, -0.08, 0.03, 0.006, -0.005, 0.095])
    p_c = torch.tensor([1.2, -0.08, 0.03, 0.004, -0.003, 0.06])      # p_a's rotation
    mocomp = {"general": (p_a, p_b, 0.25, 0.35, ts), "same_rotation": (p_a, p_c, 0.25, 0.35, ts),
              "beyond": (p_a, p_b, 0.15, 0.25, ts)}
    for name, (ps, pe, t0, t1, stamps) in mocomp.items():
        T_s, T_e = PU.tensor_to_transform(ps).float(), PU.tensor_to_transform(pe).float()
        scan = LidarScan(dirs.clone(), ranges.clone(), stamps.clone())
        scan.motion_compensate((Pose(T_s.clone()), Pose(T_e.clone())), (torch.tensor(t0), torch.tensor(t1)), Pose(T_e.clone()), False)
        out[f"mocomp_{name}_poses"] = torch.stack([T_s, T_e])
        out[f"mocomp_{name}_times"] = torch.tensor([t0, t1])
        out[f"mocomp_{name}_directions"] = scan.ray_directions
        out[f"mocomp_{name}_distances"] = scan.distances
        assert torch.equal(scan.timestamps, stamps)

    # ---- FrameSynthesis.process_lidar
    out["synthesis_times"] = np.array(SYNTHESIS_TIMES)
    for decimate in (True, False):
        settings = types.SimpleNamespace(frame_decimation_rate_hz=5, frame_match_tolerance=0.01, frame_delta_t_sec_tolerance=0.02,
                                         decimate_on_load=decimate, strategy=None, sky_removal=None)
        synth = FrameSynthesis(settings, Pose(), True)
        accepted = []
        for k, t in enumerate(SYNTHESIS_TIMES):
            stamps = torch.tensor([t, t + 0.01, t + 0.02, t + 0.03])
            synth.process_lidar(LidarScan(dirs[:, :4].clone(), ranges[:4].clone(), stamps), None)
            while synth.has_frame():
                synth.pop_frame()
                accepted.append(k)
        out[f"synthesis_accepted_decimate_{int(decimate)}"] = np.array(accepted)

    MG.save("g16_tracking", **out)


if __name__ == "__main__":
    main()
