"""DefaultLogger: listens to the tracker's frames and the mapper's keyframe updates and writes the run's trajectories in TUM format
(src/logging/default_logger.py:24-158, by member name).  Host logic only.

Under <log_directory>/trajectory/:
  tracking_only.txt          the tracker's pose of every frame
  online_estimates.txt       what was known when the frame arrived: the last keyframe update's pose of its newest keyframe, with the
                             tracker's relative motion since that keyframe's frame laid on top
  keyframe_trajectory.txt    the keyframes' poses of the last update
  estimated_trajectory.txt   every frame hung off the last keyframe at or before it:  kf_pose(r) @ inv(tracked(f_r)) @ tracked(p),
                             r the keyframe, f_r the frame it was made from.  A frame past the last keyframe hangs off the last keyframe
                             (the reference reaches the same through index -1).  One batched expression over all frames.
The last two are written only when a keyframe update arrived.  A keyframe is matched to its frame by equal start stamps."""
import os

import torch

from ..common.pose import Pose
from ..common.pose_utils import dump_trajectory_to_tum, tensor_to_transform
from ..common.signals import StopSignal


def _is_stop(value):
    return isinstance(value, StopSignal) or type(value).__name__ == "StopSignal"


def reconstruct_trajectory(tracked: torch.Tensor, stamps: torch.Tensor, kf_poses: torch.Tensor, kf_stamps: torch.Tensor) -> torch.Tensor:
    """estimated_trajectory: tracked [n,4,4] with stamps [n], keyframe poses [k,4,4] with stamps [k] (each equal to one frame's)
    -> [n,4,4]"""
    kf_frames = torch.where(stamps[:, None] == kf_stamps)[0]
    if len(kf_frames) != len(kf_stamps):
        raise ValueError(f"DefaultLogger: {len(kf_stamps)} keyframes, but {len(kf_frames)} frames carry a keyframe's stamp")
    ref = (torch.searchsorted(kf_frames, torch.arange(len(tracked)), right=True) - 1).clamp(min=0)
    return kf_poses[ref] @ (torch.linalg.inv(tracked[kf_frames[ref]]) @ tracked)


class DefaultLogger:
    def __init__(self, frame_signal, keyframe_update_signal, world_cube, calibration, log_directory: str):
        self._world_cube = world_cube
        self._frame_slot = frame_signal.register()
        self._keyframe_update_slot = keyframe_update_signal.register()
        self._timestamps = torch.Tensor([])
        self._icp_only = torch.Tensor([])              # the tracker's poses
        self._gt_path = torch.Tensor([])
        self._frame_log = torch.Tensor([])             # tracking propagated from the most recent keyframe
        self._frame_done = False
        self._gt_pose_offset = None
        self._calibration = calibration
        self._log_directory = log_directory
        self._t_world_to_kf = torch.eye(4)
        self._t_kf_to_frame = torch.eye(4)
        self._last_recv_keyframe_state = None

    def update(self) -> None:
        while self._frame_slot.has_value():
            frame = self._frame_slot.get_value()
            if self._frame_done:
                continue
            if _is_stop(frame):
                self._frame_done = True
                continue
            tracked = frame.get_lidar_pose().get_transformation_matrix().detach().cpu()
            if frame._gt_lidar_pose is not None:
                gt = frame._gt_lidar_pose.get_transformation_matrix().detach().cpu()
                if self._gt_pose_offset is None:
                    self._gt_pose_offset = torch.linalg.inv(gt)
                self._gt_path = torch.cat([self._gt_path, (self._gt_pose_offset @ gt).unsqueeze(0)])
            step = torch.linalg.inv(self._icp_only[-1]) @ tracked if len(self._icp_only) else tracked
            self._icp_only = torch.cat([self._icp_only, tracked.unsqueeze(0)])
            self._timestamps = torch.cat([self._timestamps, torch.as_tensor(frame.get_time()).detach().cpu().reshape(1).float()])
            self._t_kf_to_frame = self._t_kf_to_frame @ step
            self._frame_log = torch.cat([self._frame_log, (self._t_world_to_kf @ self._t_kf_to_frame).unsqueeze(0)])

        while self._keyframe_update_slot.has_value():
            state = self._keyframe_update_slot.get_value()
            if _is_stop(state):
                self._frame_done = True
                break
            self._last_recv_keyframe_state = state
            newest = state[-1]
            kf_frame = torch.argmin(torch.abs(self._timestamps - newest["timestamp"])).item()
            self._t_world_to_kf = Pose(pose_tensor=newest["lidar_pose"].clone()).get_transformation_matrix().detach()
            self._t_kf_to_frame = torch.linalg.inv(self._icp_only[kf_frame]) @ self._icp_only[-1]

    def finish(self) -> None:
        self.update()
        out = f"{self._log_directory}/trajectory"
        os.makedirs(out, exist_ok=True)
        dump_trajectory_to_tum(self._icp_only, self._timestamps, f"{out}/tracking_only.txt")
        dump_trajectory_to_tum(self._frame_log, self._timestamps, f"{out}/online_estimates.txt")
        state = self._last_recv_keyframe_state
        if state is not None:
            kf_stamps = torch.stack([torch.as_tensor(kf["timestamp"]).reshape(()).float() for kf in state])
            kf_poses = tensor_to_transform(torch.stack([kf["lidar_pose"] for kf in state]).float())
            dump_trajectory_to_tum(kf_poses, kf_stamps, f"{out}/keyframe_trajectory.txt")
            dump_trajectory_to_tum(reconstruct_trajectory(self._icp_only, self._timestamps, kf_poses, kf_stamps), self._timestamps,
                                   f"{out}/estimated_trajectory.txt")
