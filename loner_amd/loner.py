"""Loner: the top-level SLAM object (src/loner.py:38-278, single-process form).  Scans go in through process_lidar; the tracker
estimates each frame's pose, the mapper trains the map on the keyframes, the logger keeps the trajectories; stop() writes the
trajectory files and checkpoints/final.tar.  The log directory it leaves is the one the analysis tools of this package read.

    loner = Loner(settings)                       # settings.system.single_threaded must be True
    loner.initialize(None, gt_poses, None, ray_range, None, dataset_path, experiment_name="run")
    loner.start()
    for scan, gt_pose in sequence: loner.process_lidar(scan, gt_pose)
    loner.stop()

The multi-process mode (system.single_threaded: False) is not here: INTEGRATION.md describes running the reference's own
orchestration around this package's modules instead.  Cameras are not supported: process_rgb raises."""
import datetime
import os
import pickle
from pathlib import Path

import torch
import yaml

from .common.pose_utils import WorldCube, compute_world_cube
from .common.settings import Settings
from .common.signals import Signal
from .logging.default_logger import DefaultLogger
from .mapping.mapper import Mapper
from .tracking.tracker import Tracker


def _plain(value):
    """settings as plain Python for yaml: nested dicts and lists, tensors as numbers or lists"""
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if torch.is_tensor(value):
        return value.detach().cpu().tolist()
    return value


class Loner:
    def __init__(self, settings) -> None:
        if isinstance(settings, str):
            settings = Settings.load_from_file(settings)
        elif not isinstance(settings, dict):
            raise RuntimeError(f"Can't load settings of type {type(settings).__name__}")
        self._settings = settings
        self._single_threaded = settings.system.single_threaded
        if not self._single_threaded:
            raise NotImplementedError("Loner: system.single_threaded: False (the multi-process mode) is not implemented here; set it "
                                      "to True, or run the reference's orchestration around this package (INTEGRATION.md)")
        self._rgb_signal = Signal()
        self._lidar_signal = Signal()
        self._frame_signal = Signal()              # tracker -> mapper, logger
        self._keyframe_update_signal = Signal()    # mapper -> logger
        self._mapper = None
        self._tracker = None
        self._logger = None
        self._world_cube = None
        self._initialized = False
        self._lidar_only = settings.system.lidar_only
        if not self._lidar_only:
            raise NotImplementedError("Loner: cameras are not supported (system.lidar_only must be True)")

    def initialize(self, camera_to_lidar, all_lidar_poses, K_camera, ray_range, image_size, dataset_path: str,
                   experiment_name: str = None, config_idx: int = None, trial_idx: int = None, traj_bounding_box: dict = None) -> None:
        self._world_cube = compute_world_cube(camera_to_lidar, K_camera, image_size, all_lidar_poses, ray_range, padding=0.3,
                                              traj_bounding_box=traj_bounding_box)
        self._dataset_path = Path(dataset_path).resolve().as_posix()
        stamp = datetime.datetime.now().strftime("%m%d%y_%H%M%S")
        self._experiment_name = f"{self._settings['experiment_name'] if 'experiment_name' in self._settings else 'experiment'}_{stamp}"
        prefix = self._settings.system.log_dir_prefix
        if experiment_name is None:
            self._log_directory = os.path.expanduser(f"{prefix}/{self._experiment_name}/")
        else:
            self._log_directory = os.path.expanduser(f"{prefix}/{experiment_name}/")
            if config_idx is not None:
                self._log_directory += f"config_{config_idx}/"
            if trial_idx is not None:
                self._log_directory += f"trial_{trial_idx}/"
        os.makedirs(self._log_directory, exist_ok=True)
        self._initialized = True

    def get_world_cube(self) -> WorldCube:
        return self._world_cube

    def get_log_directory(self) -> str:
        return self._log_directory

    def start(self) -> None:
        if not self._initialized:
            raise RuntimeError("Can't Start: System Uninitialized. You must call initialize first.")
        s = self._settings
        self._logger = DefaultLogger(self._frame_signal, self._keyframe_update_signal, self._world_cube, s.calibration, self._log_directory)
        s["experiment_name"] = self._experiment_name
        s["dataset_path"] = self._dataset_path
        s["log_directory"] = self._log_directory
        s["world_cube"] = {"scale_factor": self._world_cube.scale_factor, "shift": self._world_cube.shift}
        for flag, value in s["debug"]["flags"].items():        # the debug flags, handed down
            s["debug"][flag] = bool(value and s["debug"]["global_enabled"])
        for block in ("mapper", "tracker"):
            s[block]["experiment_name"] = self._experiment_name
            s[block]["log_directory"] = self._log_directory
            s[block]["lidar_only"] = self._lidar_only
            s[block]["debug"] = s["debug"]
        if s.debug.profile or s.debug.pytorch_detect_anomaly:
            raise NotImplementedError("Loner: debug.profile and debug.pytorch_detect_anomaly are not supported")
        with open(f"{self._log_directory}/world_cube.yaml", "w+") as f:
            yaml.safe_dump(self._world_cube.as_dict(), f)
        with open(f"{self._log_directory}/full_config.yaml", "w+") as f:
            yaml.safe_dump(_plain(s), f)
        with open(f"{self._log_directory}/full_config.pkl", "wb+") as f:
            pickle.dump(s, f)
        self._mapper = Mapper(s.mapper, s.calibration, self._frame_signal, self._keyframe_update_signal, self._world_cube,
                              s.system.sky_segmentation)
        self._tracker = Tracker(s, self._rgb_signal, self._lidar_signal, self._frame_signal, device=torch.device("cuda", s.mapper.device))
        print("Starting LONER SLAM")

    def stop(self) -> None:
        self._logger.finish()
        self._mapper.finish()
        print("LONER succesfully terminated. Goodbye!")

    def _system_update(self) -> None:
        self._tracker.update()
        self._mapper.update()

    def process_lidar(self, lidar_scan, gt_pose=None) -> None:
        """One scan (time-ordered) and, optionally, its ground-truth Pose.  A scan from build_scan_from_points carries the result of
        the sortedness check the ingestion made on the device; any other scan is checked here."""
        if not getattr(lidar_scan, "time_sorted", False):
            assert torch.all(torch.diff(lidar_scan.timestamps) >= 0), "sort your points by timestamps!"
        self._logger.update()
        self._lidar_signal.emit((lidar_scan, gt_pose))
        self._system_update()

    def process_rgb(self, image) -> None:
        raise NotImplementedError("Loner.process_rgb: cameras are not supported")
