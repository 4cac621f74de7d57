"""Tracker: frame-to-frame LiDAR odometry by point-to-plane ICP (src/tracking/tracker.py:31-297), on HIP and without open3d, kornia
or pytorch3d.  Two optional settings beyond the reference's choose another estimator: icp.estimation ("POINT_TO_PLANE", the default,
or "GENERALIZED": analysis.registration's plane-to-plane ICP) and icp.robust_kernel ({type, k}; none by default).

update() takes what the rgb and lidar signals hold, lets FrameSynthesis form frames, tracks each and emits it.  track_frame builds the
frame's cloud (Frame.build_point_cloud -> ops.frame_cloud), registers it against the previous frame's cloud through the icp.schedule
(lidar_map.registration_icp, every stage starting from the one before), composes the pose in fp32 and de-skews the emitted scan
(LidarScan.motion_compensate -> ops.motion_compensate).  compute_sky_rays fills frame.lidar_points.sky_rays (ops.sky_rays).
Differences from the reference, by intent:
  * a cloud's normals are estimated once, when it becomes the ICP target (knn 30, open3d's default search); the reference also
    estimates the source's, which point-to-plane ICP never reads; with GENERALIZED a cloud gets its plane covariances once, when it
    is built (knn 20 and epsilon 1e-3, open3d's defaults), and keeps them when it becomes the target;
  * a stopped tracker ignores further update() calls;
  * run(), the multi-process orchestration and the synchronisation wait on the mapper are not here: update() is driven by the caller;
  * the debug PCD dumps (write_frame_point_clouds, write_icp_point_clouds) raise NotImplementedError when set;
  * an empty scan, a scan that is not on the device, an unknown downsample type and a non-finite pose raise.
The object holds no library handle before first use, so it pickles across a spawn as the reference's does.
"""
import copy
import time

import numpy as np
import torch

from ..common.frame import Frame
from ..common.pose import Pose
from ..common.signals import StopSignal
from .frame_synthesis import FrameSynthesis

NORMALS_KNN = 30            # open3d's estimate_normals() default: KDTreeSearchParamKNN(30)
DOWNSAMPLE_TYPES = (None, "VOXEL", "UNIFORM")
ESTIMATIONS = ("POINT_TO_PLANE", "GENERALIZED")
GICP_KNN = 20               # open3d's registration_generalized_icp: KDTreeSearchParamKNN(20) for the clouds' covariances
GICP_EPSILON = 1e-3         # TransformationEstimationForGeneralizedICP's default


def _optional(block, key, default):
    """block[key] of a settings block (a dict, or the reference's attrdict), `default` when the key is absent"""
    return block.get(key, default) if hasattr(block, "get") else getattr(block, key, default)


def robust_kernel_from_settings(entry):
    """icp.robust_kernel -> analysis.registration.RobustKernel, or None for no entry: {type: L2 | HUBER | CAUCHY | TUKEY, k: scale}"""
    from ..analysis.registration import RobustKernel
    if entry is None:
        return None
    kind, k = _optional(entry, "type", None), _optional(entry, "k", 1.0)
    if kind is None:
        raise ValueError(f"Tracker: icp.robust_kernel needs a type, got {dict(entry)!r}")
    return RobustKernel(str(kind).lower(), k)


def _is_stop(value):
    return isinstance(value, StopSignal) or type(value).__name__ == "StopSignal"


class Tracker:
    def __init__(self, settings, rgb_signal, lidar_signal, frame_signal, device=None) -> None:
        self._rgb_slot = rgb_signal.register()
        self._lidar_slot = lidar_signal.register()
        self._frame_signal = frame_signal
        self._settings = settings.tracker
        self._t_lidar_to_camera = Pose.from_settings(settings.calibration.lidar_to_camera)
        self._lidar_only = settings.system.lidar_only
        self._frame_synthesizer = FrameSynthesis(self._settings.frame_synthesis, self._t_lidar_to_camera, self._lidar_only)
        self._device = device
        self._processed_stop_signal = False

        # frame-to-frame tracking state
        self._reference_point_cloud = None
        self._reference_pose = Pose(fixed=True)
        self._reference_time = None

        self._frame_count = 0
        self._last_tracked_frame_time = 0
        self.last_registrations = []          # the RegistrationResult of every stage of the last tracked frame

        debug = self._settings.debug
        for flag in ("write_frame_point_clouds", "write_icp_point_clouds"):
            if getattr(debug, flag, False):
                raise NotImplementedError(f"Tracker: debug.{flag} (PCD dumps) is not supported")
        if self._settings.icp.downsample.type not in DOWNSAMPLE_TYPES:
            raise ValueError(f"Unrecognized downsample type {self._settings.icp.downsample.type}")
        self._estimation = _optional(self._settings.icp, "estimation", "POINT_TO_PLANE")
        if self._estimation not in ESTIMATIONS:
            raise ValueError(f"Unrecognized icp.estimation {self._estimation!r} (one of {ESTIMATIONS})")
        self._robust_kernel = robust_kernel_from_settings(_optional(self._settings.icp, "robust_kernel", None))

    def update(self) -> None:
        """One turn of the tracker: take at most one value from each input signal, then track and emit every frame that is ready.
        A StopSignal on either input ends the tracker: that turn and every later one do nothing."""
        if self._processed_stop_signal:
            print("Tracker.update: the tracker has been stopped")
            return
        started = time.time()
        feeds = ((self._rgb_slot, self._frame_synthesizer.process_image),
                 (self._lidar_slot, lambda scan_and_pose: self._frame_synthesizer.process_lidar(*scan_and_pose)))
        for slot, feed in feeds:
            if not slot.has_value():
                continue
            value = slot.get_value()
            if _is_stop(value):
                self._processed_stop_signal = True
                return
            feed(value)
        emitted = self._emit_ready_frames()
        if emitted and self._settings.debug.log_times:
            with open(f"{self._settings.log_directory}/track_times.csv", "a+") as log:
                log.write(f"{time.time() - started},{emitted}\n")

    def _emit_ready_frames(self) -> int:
        """Tracks what FrameSynthesis has finished, in order; a frame gets the next id only when it is emitted.  -> frames emitted"""
        emitted = 0
        while self._frame_synthesizer.has_frame():
            frame = self._frame_synthesizer.pop_frame()
            frame._id = self._frame_count
            if not self.track_frame(frame):
                print(f"Tracker: frame at {frame.get_time()} could not be tracked and is skipped")
                continue
            if self._settings.compute_sky_rays:
                self.compute_sky_rays(frame)
            self._frame_signal.emit(frame)
            self._last_tracked_frame_time = frame.get_time()
            self._frame_count += 1
            emitted += 1
        return emitted

    def _place(self, frame: Frame) -> None:
        """A frame off the signals may still be on the host: with a device given, move it there"""
        if self._device is not None:
            frame.to(self._device)
        scan = frame.lidar_points
        if len(scan) == 0:
            raise ValueError("Tracker: the frame's scan is empty")
        if not scan.timestamps.is_cuda:
            raise RuntimeError(f"Tracker: the scan is on {scan.timestamps.device}; tracking runs on the device (pass device=, or move "
                               "the frame)")

    def frame_cloud(self, frame: Frame):
        """The cloud ICP sees of a frame: the middle icp.scan_duration share of the scan, thinned as icp.downsample says (None: every
        point; VOXEL: one mean per voxel; UNIFORM: every k-th point, about target_uniform_point_count in all)."""
        icp = self._settings.icp
        kind = icp.downsample.type
        if kind not in DOWNSAMPLE_TYPES:
            raise ValueError(f"Unrecognized downsample type {kind}")
        wanted = icp.downsample.target_uniform_point_count if kind == "UNIFORM" else None
        cloud = frame.build_point_cloud(scan_duration=icp.scan_duration, target_points=wanted)
        cloud = cloud.voxel_down_sample(icp.downsample.voxel_downsample_size) if kind == "VOXEL" else cloud
        if self._estimation == "GENERALIZED":
            from ..analysis.registration import cloud_covariances
            cloud.covariances = cloud_covariances(cloud, GICP_EPSILON, GICP_KNN)
        return cloud

    def _register(self, cloud) -> np.ndarray:
        """The rigid motion (fp64 4x4) that lays `cloud` onto the reference cloud: icp.schedule from the identity, coarse to fine, every
        stage starting where the one before ended.  The stages' results stay in last_registrations."""
        from ..analysis.lidar_map import registration_icp
        from ..analysis.registration import registration_generalized_icp, registration_icp_robust
        motion = np.eye(4)
        self.last_registrations = []
        for stage in self._settings.icp.schedule:
            args = (cloud, self._reference_point_cloud, stage.threshold, motion, stage.relative_fitness, stage.relative_rmse,
                    stage.max_iterations)
            if self._estimation == "GENERALIZED":
                result = registration_generalized_icp(*args, kernel=self._robust_kernel, epsilon=GICP_EPSILON, knn=GICP_KNN)
            elif self._robust_kernel is not None:
                result = registration_icp_robust(*args, kernel=self._robust_kernel)
            else:
                result = registration_icp(*args)
            self.last_registrations.append(result)
            motion = result.transformation.copy()
        if not np.isfinite(motion).all():
            raise ValueError("Tracker: the registration is not finite")
        return motion

    def _become_reference(self, cloud, pose_matrix, stamp) -> None:
        """The next frame is registered against this one: its cloud as built (never the compensated scan), with the normals
        point-to-plane ICP needs of a target (generalized ICP reads the covariances the cloud was built with), its pose (kept on the
        host) and its middle time."""
        self._reference_point_cloud = cloud if self._estimation == "GENERALIZED" else cloud.estimate_normals(NORMALS_KNN)
        self._reference_pose = Pose(pose_matrix, fixed=True)
        self._reference_time = stamp

    def track_frame(self, frame: Frame) -> bool:
        """Estimates the frame's pose, stores it in the frame and de-skews the frame's scan; True when tracked.  The first frame is the
        fixed origin.  Every later one is registered against its predecessor and its pose is predecessor_pose @ registration, an fp32
        product of two 4x4 matrices formed on the host, where the registration arrives; the frame's own copy goes to the device once."""
        self._place(frame)
        cloud = self.frame_cloud(frame)
        device = frame.lidar_points.timestamps.device
        stamp = frame.get_middle_time()
        if self._reference_point_cloud is None:
            origin = self._reference_pose.get_transformation_matrix().detach().clone()
            frame._lidar_pose = Pose(origin.clone(), fixed=True, requires_tensor=True).to(device)
            self.last_registrations = []
            self._become_reference(cloud, origin, stamp)
            return True

        pose_matrix = self._reference_pose.get_transformation_matrix().detach() @ torch.from_numpy(self._register(cloud)).float()
        host_pose = Pose(pose_matrix.clone(), requires_tensor=True)
        frame._lidar_pose = copy.deepcopy(host_pose).to(device)
        if self._settings.motion_compensation.enabled:           # both poses are on the host: only the two times are read back
            frame.lidar_points.motion_compensate((self._reference_pose, host_pose), (self._reference_time, stamp), host_pose,
                                                 self._settings.motion_compensation.use_gpu)
        self._become_reference(cloud, pose_matrix, stamp)
        return True

    def compute_sky_rays(self, frame: Frame) -> None:
        """frame.lidar_points.sky_rays: the world-frame directions the scan saw nothing along (tracker.py:257-297)."""
        from .. import ops
        scan = frame.lidar_points
        if len(scan) == 0:
            raise ValueError("compute_sky_rays: the frame's scan is empty")
        rotation = frame.get_lidar_pose().get_rotation().detach()
        if not bool(torch.isfinite(rotation).all()):
            raise ValueError("compute_sky_rays: the frame's pose is not finite")
        scan.sky_rays = ops.sky_rays(scan.ray_directions, rotation)
