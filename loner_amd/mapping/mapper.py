"""Mapper: takes the tracker's frames, lets the KeyFrameManager choose keyframes, runs the Optimizer on the active window and writes
the checkpoints the analysis tools read (src/mapping/mapper.py:30-180, single-process form).

update() handles at most one frame.  With optimizer.enabled and a keyframe to train on it runs Optimizer.iterate_optimizer on the
window, writes checkpoints/ckpt_<kf_idx>.tar (kf_idx = the optimiser's keyframe count - 1) and emits the keyframes' pose states on the
keyframe-update signal.  The checkpoint is the full one (build_ckpt) after every keyframe when log_level is VERBOSE and after every
tenth when it is STANDARD; otherwise it holds {'global_step', 'poses'} only.  With optimizer.enabled off the poses alone are saved
every hundredth frame.  debug.use_groundtruth_poses replaces a frame's pose by its ground truth before anything looks at it;
debug.log_times appends the wall time of every mapped frame to map_times.csv.  finish() writes checkpoints/final.tar.
There is no run() loop and no shared state: the caller drives update(), as with Tracker.  A stopped mapper ignores further calls."""
import os
import time

import torch

from ..common.signals import StopSignal
from .keyframe_manager import KeyFrameManager
from .optimizer import Optimizer


def _is_stop(value):
    return isinstance(value, StopSignal) or type(value).__name__ == "StopSignal"


class Mapper:
    def __init__(self, settings, calibration, frame_signal, keyframe_update_signal, world_cube, enable_sky_segmentation: bool = True,
                 optimizer_factory=Optimizer) -> None:
        """optimizer_factory: what builds the optimiser, with Optimizer's argument list (the host tests count calls with a stub)"""
        self._frame_slot = frame_signal.register()
        self._keyframe_update_signal = keyframe_update_signal
        self._settings = settings
        self._lidar_only = settings.lidar_only
        self._world_cube = world_cube
        for block in ("keyframe_manager", "optimizer"):
            settings[block]["debug"] = settings.debug
            settings[block]["log_directory"] = settings.log_directory
        self._keyframe_manager = KeyFrameManager(settings.keyframe_manager, "cpu" if settings.data_prep_on_cpu else settings.device)
        self._optimizer = optimizer_factory(settings.optimizer, calibration, world_cube, 0, settings.debug.use_groundtruth_poses,
                                            self._lidar_only, enable_sky_segmentation)
        self._processed_stop_signal = False
        os.makedirs(f"{settings.log_directory}/checkpoints", exist_ok=True)

    def _checkpoint_path(self, name) -> str:
        return f"{self._settings.log_directory}/checkpoints/{name}.tar"

    def update(self) -> None:
        if self._processed_stop_signal:
            print("Not updating mapper: Mapping already done.")
            return
        if not self._frame_slot.has_value():
            return
        started = time.time()
        frame = self._frame_slot.get_value()
        if _is_stop(frame):
            self._processed_stop_signal = True
            return
        if self._settings.debug.use_groundtruth_poses:
            frame._lidar_pose = frame._gt_lidar_pose
        keyframe = self._keyframe_manager.process_frame(frame)
        if not self._settings.optimizer.enabled:
            if self._optimizer._global_step % 100 == 0:
                torch.save({"poses": self._keyframe_manager.get_poses_state()}, self._checkpoint_path(f"ckpt_{self._optimizer._keyframe_count}"))
            self._optimizer._global_step += 1
            return
        if keyframe is None:
            return
        self._optimizer.iterate_optimizer(self._keyframe_manager.get_active_window())
        pose_state = self._keyframe_manager.get_poses_state()
        kf_idx = self._optimizer._keyframe_count - 1
        level = self._settings.log_level
        level = level[0] if isinstance(level, tuple) else level
        if level == "VERBOSE" or (level == "STANDARD" and kf_idx % 10 == 0):
            checkpoint = self.build_ckpt()
        else:
            checkpoint = {"global_step": self._optimizer._global_step, "poses": pose_state}
        torch.save(checkpoint, self._checkpoint_path(f"ckpt_{kf_idx}"))
        self._keyframe_update_signal.emit(pose_state)
        if self._settings.debug.log_times:
            with open(f"{self._settings.log_directory}/map_times.csv", "a+") as log:
                log.write(f"{time.time() - started}\n")

    def build_ckpt(self) -> dict:
        opt = self._optimizer
        checkpoint = {"global_step": opt._global_step, "network_state_dict": opt._model.state_dict(),
                      "optimizer_state_dict": opt._optimizer.state_dict(), "poses": self._keyframe_manager.get_poses_state()}
        if self._settings.optimizer.samples_selection.strategy == "OGM":
            checkpoint["occ_model_state_dict"] = opt._occupancy_grid_model.state_dict()
            checkpoint["occ_optimizer_state_dict"] = opt._occupancy_grid_optimizer.state_dict()
        return checkpoint

    def finish(self) -> None:
        print("Saving Last Checkpoint to", self._checkpoint_path("final"))
        torch.save(self.build_ckpt(), self._checkpoint_path("final"))
