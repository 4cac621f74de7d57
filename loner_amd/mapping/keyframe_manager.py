"""KeyFrameManager: decides which tracked frames become keyframes, carries the optimised pose of the last keyframe over to a new one,
and picks the window the optimiser trains on (src/mapping/keyframe_manager.py:23-194, by member name).  Host logic only.

Selection.  The temporal criterion holds when the frame starts at least temporal.time_diff_seconds after the last accepted time; the
motion criterion when the frame's tracked pose has moved motion.translation_threshold_m or turned motion.rotation_threshold_deg away
from the last keyframe's (optimised) pose.  The first frame meets both.
  TEMPORAL      a keyframe when the temporal criterion holds
  MOTION        a keyframe when the motion criterion holds
  HYBRID        a keyframe when both hold; when only the temporal one holds the accepted time still advances and the LAST keyframe is
                returned again, so the mapper trains on while the sensor stands still
  HYBRID_LAZY   a keyframe when both hold, nothing otherwise; get_last_mapped_time() still advances past frames that were refused
                for lack of motion (MOTION does the same)
Pose.  A new keyframe starts from optimised(ref) @ inv(tracked(ref)) @ tracked(new), ref being the keyframe before it: the tracker's
relative motion laid onto what the optimiser made of the reference.
Window.  MOST_RECENT: the last window_size keyframes.  RANDOM / HYBRID: r recent keyframes (1, or hybrid_settings.num_recent_frames;
at most the window and the keyframes there are) and window_size - r of the K - r older ones, drawn as torch.randperm(K - r)[:w - r]
from torch's CPU generator; the recent ones come LAST (the optimiser's sample allocation relies on that).
"""
from enum import Enum
from typing import List, Optional

import torch

from ..common.frame import Frame
from ..common.pose import Pose
from .keyframe import KeyFrame


class KeyFrameSelectionStrategy(Enum):
    TEMPORAL = 0
    MOTION = 1
    HYBRID = 2
    HYBRID_LAZY = 3


class WindowSelectionStrategy(Enum):
    MOST_RECENT = 0
    RANDOM = 1
    HYBRID = 2


def propagated_pose(optimised_reference: torch.Tensor, tracked_reference: torch.Tensor, tracked_new: torch.Tensor) -> torch.Tensor:
    """optimised(ref) @ inv(tracked(ref)) @ tracked(new), 4x4 matrices"""
    return optimised_reference @ (torch.linalg.inv(tracked_reference) @ tracked_new)


class KeyFrameManager:
    def __init__(self, settings, device="cpu") -> None:
        self._settings = settings
        self._keyframe_selection_strategy = KeyFrameSelectionStrategy[settings.keyframe_selection.strategy]
        self._window_selection_strategy = WindowSelectionStrategy[settings.window_selection.strategy]
        self._device = device
        self._last_accepted_frame_ts = None
        self._last_motion_rejected_frame_ts = None       # a frame old enough to map that had not moved enough
        self._keyframes: List[KeyFrame] = []
        self._global_step = 0

    def __len__(self) -> int:
        return len(self._keyframes)

    # ---- selection
    def _select_frame_temporal(self, frame: Frame) -> bool:
        if not self._keyframes:
            return True
        return bool(frame.get_time() - self._last_accepted_frame_ts >= self._settings.keyframe_selection.temporal.time_diff_seconds)

    def _select_frame_motion(self, frame: Frame) -> bool:
        if not self._keyframes:
            return True
        moved = self._keyframes[-1].get_lidar_pose().inv() * frame.get_lidar_pose()
        limits = self._settings.keyframe_selection.motion
        distance = moved.get_translation().norm()
        angle = moved.get_axis_angle().rad2deg().norm()
        return bool(distance >= limits.translation_threshold_m or angle >= limits.rotation_threshold_deg)

    def _add_keyframe(self, frame: Frame) -> KeyFrame:
        keyframe = KeyFrame(frame, self._device)
        if self._keyframes:
            ref = self._keyframes[-1]
            matrix = lambda pose: pose.get_transformation_matrix().detach()
            start = propagated_pose(matrix(ref.get_lidar_pose()), matrix(ref._tracked_lidar_pose), matrix(keyframe._tracked_lidar_pose))
            keyframe._frame._lidar_pose = Pose(start, requires_tensor=True)
        self._keyframes.append(keyframe)
        return keyframe

    def process_frame(self, frame: Frame) -> Optional[KeyFrame]:
        """-> the keyframe the mapper should train on now (a new one, or under HYBRID the last one again), or None"""
        strategy = self._keyframe_selection_strategy
        temporal = self._select_frame_temporal(frame)
        if strategy == KeyFrameSelectionStrategy.TEMPORAL:
            accept = temporal
        else:
            motion = self._select_frame_motion(frame)
            if temporal and not motion:
                self._last_motion_rejected_frame_ts = frame.get_time()
            accept = motion if strategy == KeyFrameSelectionStrategy.MOTION else (motion and temporal)
        keyframe = None
        if accept:
            self._last_accepted_frame_ts = frame.get_time()
            keyframe = self._add_keyframe(frame)
        if strategy == KeyFrameSelectionStrategy.HYBRID:
            if temporal:
                self._last_accepted_frame_ts = frame.get_time()
            return self._keyframes[-1] if temporal else None
        return keyframe

    def get_last_mapped_time(self):
        lazy = self._keyframe_selection_strategy in (KeyFrameSelectionStrategy.HYBRID_LAZY, KeyFrameSelectionStrategy.MOTION)
        if lazy and self._last_motion_rejected_frame_ts is not None:
            return max(self._last_motion_rejected_frame_ts, self._last_accepted_frame_ts)
        return self._last_accepted_frame_ts

    # ---- access
    def get_keyframes(self, idxs=None) -> List[KeyFrame]:
        return self._keyframes if idxs is None else [self._keyframes[i] for i in idxs]

    def get_active_window(self) -> List[KeyFrame]:
        size = self._settings.window_selection.window_size
        strategy = self._window_selection_strategy
        if strategy == WindowSelectionStrategy.MOST_RECENT:
            return self._keyframes[-size:]
        if strategy not in (WindowSelectionStrategy.RANDOM, WindowSelectionStrategy.HYBRID):
            raise ValueError(f"Can't use unknown WindowSelectionStrategy {strategy}")
        count = len(self._keyframes)
        recent = 1 if strategy == WindowSelectionStrategy.RANDOM else self._settings.window_selection.hybrid_settings.num_recent_frames
        recent = min(recent, count, size)
        older = torch.randperm(count - recent)[:size - recent].tolist()
        return [self._keyframes[i] for i in older + list(range(count - recent, count))]

    def get_poses_state(self) -> List[dict]:
        return [keyframe.get_pose_state() for keyframe in self._keyframes]
