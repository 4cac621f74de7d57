"""FrameSynthesis: turns the streams of scans and images into Frames, behind the class surface of the reference's
src/tracking/frame_synthesis.py (process_lidar, process_image, create_frames, has_frame, pop_frame).  Host logic only.

Contract.
  * Decimation: a stamp is *due* when it lies at least one frame period, less frame_delta_t_sec_tolerance, after the last accepted one.
  * Lidar only: a scan becomes a frame when decimate_on_load is set (the loader has thinned the stream already) or when its start
    time is due.  The frame holds copies of the scan, the calibration and the ground-truth pose.
  * With images: a due image opens a frame that waits for its scan.  Scans wait in arrival order with their time range widened by
    frame_match_tolerance on both sides.  Images and scans both arrive in time order, so matching is a single forward walk: scans
    that ended before the image can serve no later image either and are discarded; if the oldest remaining scan has begun by the
    image's time it is the match and is consumed; if it begins later the image can never be matched and its frame is dropped; with
    no scan left the image keeps waiting.  A matched frame whose scan is empty is not handed out.
"""
import collections
from typing import Optional

from ..common.frame import Frame
from ..common.pose import Pose
from ..common.sensors import LidarScan

_WaitingScan = collections.namedtuple("_WaitingScan", "begin end scan gt_pose")


def _copy(member):
    return None if member is None else member.clone()


class FrameSynthesis:
    def __init__(self, settings, T_lidar_to_camera: Pose, lidar_only: bool) -> None:
        self._settings = settings
        self._t_lidar_to_camera = T_lidar_to_camera
        self._t_camera_to_lidar = T_lidar_to_camera.inv()
        self._lidar_only = lidar_only
        self._decimate_on_load = settings.decimate_on_load
        self._min_spacing = 1.0 / settings.frame_decimation_rate_hz - settings.frame_delta_t_sec_tolerance
        self._match_slack = settings.frame_match_tolerance
        self._last_accepted = float("-inf")
        self._image_frames = collections.deque()      # frames that hold an image and wait for a scan, oldest first
        self._lidar_scans = collections.deque()       # _WaitingScan, oldest first
        self._ready = collections.deque()

    def _due(self, stamp) -> bool:
        return bool(stamp - self._last_accepted >= self._min_spacing)

    # ---- input
    def process_lidar(self, lidar_scan: LidarScan, gt_pose: Optional[Pose]) -> None:
        if not self._lidar_only:
            stamps = lidar_scan.timestamps
            self._lidar_scans.append(_WaitingScan(float(stamps[0]) - self._match_slack, float(stamps[-1]) + self._match_slack,
                                                  lidar_scan, gt_pose))
            self.create_frames()
            return
        begin = lidar_scan.get_start_time()
        if self._decimate_on_load or self._due(begin):
            frame = Frame(None, lidar_scan.clone(), _copy(self._t_lidar_to_camera))
            frame._gt_lidar_pose = _copy(gt_pose)
            self._ready.append(frame)
            self._last_accepted = begin

    def process_image(self, image) -> None:
        """Images must arrive in increasing time order."""
        if self._due(image.timestamp):
            self._last_accepted = image.timestamp
            self._image_frames.append(Frame(_copy(image), None, _copy(self._t_lidar_to_camera)))
            self.create_frames()

    # ---- matching
    def create_frames(self) -> None:
        while self._image_frames:
            stamp = float(self._image_frames[0].image.timestamp)
            while self._lidar_scans and self._lidar_scans[0].end < stamp:
                self._lidar_scans.popleft()
            if not self._lidar_scans:
                return                                 # the image waits for scans still to come
            frame = self._image_frames.popleft()
            if self._lidar_scans[0].begin > stamp:
                print(f"FrameSynthesis: no scan covers the image at {stamp}; its frame is dropped")
                continue
            match = self._lidar_scans.popleft()
            frame.lidar_points, frame._gt_lidar_pose = match.scan, match.gt_pose
            if len(match.scan) > 0:
                self._ready.append(frame)

    # ---- output
    def has_frame(self) -> bool:
        return len(self._ready) > 0

    def pop_frame(self) -> Optional[Frame]:
        """The oldest finished frame, or None."""
        return self._ready.popleft() if self._ready else None
