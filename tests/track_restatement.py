"""CPU restatement of the tracker's contract (include/loner_hip.h, "tracking"; loner_amd/tracking/tracker.py): the frame cloud's
window and points with the reference's scalar-meets-tensor casts, motion compensation in fp64, the sky mask op for op in torch fp32 (the
closing as two padded max-pools: kornia is not installed, this IS its definition here), the ICP chain on tests/icp_restatement.py, and
a generator of motion-distorted scans of the analytic scene."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from loner_amd.common.pose_utils import matrix_to_axis_angle, tensor_to_transform
from loner_amd.utils import synthetic as SY
from tests import cloud_restatement as CR
from tests import icp_restatement as IR

NUMERIC_TOLERANCE = 1e-9
TOP_ROWS = 3
HORIZON_OFFSET = 10


# ---------------------------------------------------------------- frame cloud
def cloud_window(timestamps, scan_duration=None, target_points=None):
    """(start, stop, step) of Frame.build_point_cloud's slice, on a CPU tensor of sorted timestamps.  With a scan_duration and a scan
    longer than 1e-3 s the window is centred on the mean of the first and last stamp and half = scan_duration * (last - first) / 2
    wide on either side, half being a Python float that torch casts to the stamps' type where it meets them: start is the first
    stamp at or after centre - half, stop the first at or after centre + half, or the scan's length when the last stamp lies below
    centre + half.  step thins the window to about target_points."""
    stamps = timestamps.detach().cpu()
    count = len(stamps)
    first, last = stamps[0], stamps[-1]
    begin, end = 0, count
    if scan_duration is not None and bool(last - first > 1e-3):
        half = scan_duration * float(last - first) / 2
        centre = (first + last) / 2
        offset = stamps - centre
        first_true = lambda mask: int(torch.nonzero(mask)[0]) if bool(mask.any()) else 0
        begin = first_true(offset >= -half)
        end = count if bool(last < centre + half) else first_true(offset >= half)
    step = 1 if target_points is None else (end - begin) // target_points
    return begin, end, step or 1


def frame_cloud(directions, distances, timestamps, scan_duration=None, target_points=None):
    """-> (start, stop, step, points fp64 [m,3]): the fp32 products widened, the array the reference hands to open3d"""
    a, b, s = cloud_window(timestamps, scan_duration, target_points)
    pts = directions.detach().cpu()[..., a:b:s] * distances.detach().cpu()[a:b:s]
    return a, b, s, pts.numpy().transpose().astype(np.float64)


# ---------------------------------------------------------------- motion compensation
def motion_compensate(directions, distances, timestamps, T_start, T_end, t_start, t_end, T_target):
    """sensors.py:176-232 with everything after the interpolation factor in fp64 -> (directions [3,n], distances [n]) in fp64, not
    rounded.  The factor is formed in the timestamps' type as the reference forms it; the pose matrices (fp32) are widened; the
    relative axis-angle is the package's matrix_to_axis_angle of R_start^-1 R_end in fp64; exp() is scipy's rotation vector map."""
    from scipy.spatial.transform import Rotation
    ts = timestamps.detach().cpu()
    t0 = torch.as_tensor(t_start).detach().cpu() if torch.is_tensor(t_start) else t_start
    t1 = torch.as_tensor(t_end).detach().cpu() if torch.is_tensor(t_end) else t_end
    f = ((ts - t0) / (t1 - t0)).double().numpy()
    Ts, Te, Tt = (np.asarray(T.detach().cpu().numpy() if torch.is_tensor(T) else T, dtype=np.float64) for T in (T_start, T_end, T_target))
    trans = Ts[:3, 3] + f[:, None] * (Te[:3, 3] - Ts[:3, 3])
    rel = np.linalg.inv(Ts[:3, :3]) @ Te[:3, :3]
    aa = matrix_to_axis_angle(torch.from_numpy(rel)).numpy()
    theta = np.linalg.norm(aa)
    if theta < NUMERIC_TOLERANCE:
        R = np.tile(Ts[:3, :3], (len(f), 1, 1))
    else:
        R = Ts[:3, :3] @ Rotation.from_rotvec(f[:, None] * aa[None, :]).as_matrix()
    p = directions.detach().cpu().double().numpy() * distances.detach().cpu().double().numpy()
    world = np.einsum("nab,bn->na", R, p) + trans
    Ti = np.linalg.inv(Tt)
    q = world @ Ti[:3, :3].T + Ti[:3, 3]
    dist = np.linalg.norm(q, axis=1)
    return (q / dist[:, None]).T, dist


# ---------------------------------------------------------------- sky rays (include/loner_hip.h: lnr_sky_rays)
SKY_COLUMNS = 360


def integer_degrees(directions):
    """-> (azimuth, polar) int64 [n]: the whole degrees (round half to even, in fp32) of atan2(y, x) and of the angle from +z"""
    d = directions.detach().cpu().float()
    planar = torch.sqrt(d[0] * d[0] + d[1] * d[1])
    whole = lambda angle: torch.rad2deg(angle).round().to(torch.int64)
    return whole(torch.atan2(d[1], d[0])), whole(torch.atan2(planar, d[2]))


def sky_image(directions):
    """-> (image fp32 [rows, 360] with 1 where a direction falls, polar_min, azimuth_min): one row per whole polar degree from the
    smallest to the largest seen, one column per azimuth degree counted from the smallest seen; column 360 is column 0 again."""
    azimuth, polar = integer_degrees(directions)
    polar_min, azimuth_min = int(polar.min()), int(azimuth.min())
    rows = int(polar.max()) - polar_min + 1
    image = torch.zeros(rows * SKY_COLUMNS)
    image[(polar - polar_min) * SKY_COLUMNS + (azimuth - azimuth_min) % SKY_COLUMNS] = 1
    return image.reshape(rows, SKY_COLUMNS), polar_min, azimuth_min


def closing(depth_img):
    """a 3x3 dilation then a 3x3 erosion, out-of-image neighbours ignored (max_pool2d pads with -inf), and the top rows set"""
    img = depth_img[None, None]
    img = F.max_pool2d(img, 3, stride=1, padding=1)
    img = -F.max_pool2d(-img, 3, stride=1, padding=1)
    img = img[0, 0].clone()
    img[:TOP_ROWS] = 1
    return img


def empty_pixel_directions(image, polar_min, azimuth_min, rotation):
    """-> (rotated unit vectors [3,k] fp32 of the zero pixels in row-major order, their elevation above the horizon in degrees): pixel
    (r, c) stands for the polar angle r + polar_min and the azimuth c + azimuth_min, whole degrees turned to radians in fp32"""
    pixels = torch.nonzero(image == 0)                        # row-major
    polar = torch.deg2rad((pixels[:, 0] + polar_min).float())
    azimuth = torch.deg2rad((pixels[:, 1] + azimuth_min).float())
    units = torch.stack((torch.sin(polar) * torch.cos(azimuth), torch.sin(polar) * torch.sin(azimuth), torch.cos(polar)))
    turned = rotation.detach().cpu().float() @ units
    elevation = 90 - torch.rad2deg(torch.atan2(torch.sqrt(turned[0] * turned[0] + turned[1] * turned[1]), turned[2]))
    return turned, elevation


def sky_rays(directions, rotation):
    """-> (sky rays [3,m] fp32: the empty pixels' directions more than HORIZON_OFFSET degrees above the horizon, in pixel order; a dict
    of diagnostics: candidates, rows, the smallest distance of a direction's degrees to a half-integer (taken in fp64), the smallest
    distance of a candidate's elevation to the cut)"""
    image, polar_min, azimuth_min = sky_image(directions)
    turned, elevation = empty_pixel_directions(closing(image), polar_min, azimuth_min, rotation)
    x, y, z = directions.detach().cpu().double()
    deg = torch.cat([torch.atan2(y, x).rad2deg(), torch.atan2(torch.sqrt(x ** 2 + y ** 2), z).rad2deg()])
    tie = float(((deg - torch.floor(deg)) - 0.5).abs().min())
    cut = float((elevation - HORIZON_OFFSET).abs().min()) if elevation.numel() else float("inf")
    return turned[:, elevation > HORIZON_OFFSET], {"candidates": int(elevation.numel()), "tie_margin_deg": tie, "cut_margin_deg": cut,
                                                   "rows": int(image.shape[0])}


def sky_case():
    """(directions [3,n] fp32, rotation [3,3] fp32) of the sky-ray tests: SY.lidar_pattern(fov_deg=(-15.2, 22.3)) with the azimuths
    turned by 0.2071 degrees in fp64 before the cast (the default pattern puts beams and azimuth columns exactly on half-integer
    degrees), returns dropped above 4 degrees elevation for azimuths in (-60, 75) and above 12 degrees for azimuths beyond 120, and a
    pose of yaw 3.7, pitch -2.1."""
    beams, azimuths = 64, 1024
    el = torch.deg2rad(torch.linspace(-15.2, 22.3, beams, dtype=torch.float64))
    az = 2 * math.pi * torch.arange(azimuths, dtype=torch.float64) / azimuths + math.radians(0.2071)
    ce, se = torch.cos(el)[:, None], torch.sin(el)[:, None]
    d = torch.stack([ce * torch.cos(az)[None, :], ce * torch.sin(az)[None, :], se.expand(-1, azimuths)], 0).reshape(3, -1)
    el_deg = torch.rad2deg(el)[:, None].expand(-1, azimuths).reshape(-1)
    az_deg = torch.rad2deg(torch.atan2(d[1], d[0]))
    drop = ((el_deg > 4) & (az_deg > -60) & (az_deg < 75)) | ((el_deg > 12) & (az_deg > 120))
    y, p = math.radians(3.7), math.radians(-2.1)
    Rz = torch.tensor([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    Ry = torch.tensor([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    return d[:, ~drop].float().contiguous(), (Rz @ Ry).float()


def open_sky(directions, distances, timestamps):
    """a scan with the returns above 12 degrees of elevation dropped for azimuths in (-60, 75): the closed analytic scene returns on
    every ray, this opens a patch of sky"""
    el, az = torch.rad2deg(torch.asin(directions[2])), torch.rad2deg(torch.atan2(directions[1], directions[0]))
    keep = ~((el > 12) & (az > -60) & (az < 75))
    return directions[:, keep].contiguous(), distances[keep].contiguous(), timestamps[keep].contiguous()


# ---------------------------------------------------------------- fixture G16
def g16():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_tracking.npz"))


def g16_cloud_args(g, name):
    """(scan_duration, target_points) of the recorded build_point_cloud case `name`"""
    duration, target = g[f"cloud_{name}_args"]
    return (None if np.isnan(duration) else float(duration)), (None if target < 0 else int(target))


def g16_mocomp_errors(g, name, dirs_of, dist_of):
    """max |distance error| and max |direction component error| of a result against the fp64 restatement of the recorded case `name`,
    and that restatement"""
    dirs, dist, ts = (torch.from_numpy(g[k]) for k in ("directions", "distances", "timestamps"))
    T_s, T_e = torch.from_numpy(g[f"mocomp_{name}_poses"])
    t0, t1 = torch.from_numpy(g[f"mocomp_{name}_times"])
    want_dirs, want_dist = motion_compensate(dirs, dist, ts, T_s, T_e, t0, t1, T_e)
    return (float(np.abs(dist_of.astype(np.float64) - want_dist).max()), float(np.abs(dirs_of.astype(np.float64) - want_dirs).max()),
            want_dirs, want_dist)


def g16_world_magnitude(g):
    """the largest world-frame coordinate of the fixture's points: what the reference's fp32 chain rounds at"""
    p = g["directions"].astype(np.float64) * g["distances"].astype(np.float64)
    big = 0.0
    for name in ("general", "same_rotation", "beyond"):
        for T in g[f"mocomp_{name}_poses"].astype(np.float64):
            big = max(big, float(np.abs(T[:3, :3] @ p + T[:3, 3:4]).max()))
    return big


# ---------------------------------------------------------------- the ICP chain
def normals(points, knn=30):
    idx, _ = IR.knn(points, knn)
    return IR.normal_rule(IR.covariance(points, idx))[0]


def icp_stage(source, target, target_normals, stage, init):
    """one entry of icp.schedule from init -> IR.icp's dict"""
    return IR.icp(source, target, target_normals, float(stage["threshold"]), init=np.array(init, dtype=np.float64),
                  relative_fitness=float(stage["relative_fitness"]), relative_rmse=float(stage["relative_rmse"]),
                  max_iteration=int(stage["max_iterations"]), corr=IR.correspondences_grid)


def track_chain(clouds, schedule, target_normals=None):
    """Frame-to-frame tracking of a list of clouds (numpy [n,3]): -> (poses fp32 [k,4,4] torch, registrations: per frame the list of
    IR.icp dicts).  The first pose is the identity; pose_k = pose_{k-1} @ fp32(registration), composed in fp32."""
    poses = [torch.eye(4)]
    regs = [[]]
    for k in range(1, len(clouds)):
        tgt = clouds[k - 1]
        nrm = normals(tgt) if target_normals is None else target_normals[k - 1]
        T = np.eye(4)
        stages = []
        for stage in schedule:
            out = icp_stage(clouds[k], tgt, nrm, stage, T)
            stages.append(out)
            T = out["transformation"].copy()
        regs.append(stages)
        poses.append(poses[-1] @ torch.from_numpy(T).float())
    return torch.stack(poses), regs


# ---------------------------------------------------------------- motion-distorted scans
def pose_at(t, speed=3.0, yaw_rate_deg=20.0):
    """[n,4,4] fp64: the sensor's pose at times t along SY.trajectory_pose6-like motion (a straight line along x at `speed` m/s,
    turning about z at `yaw_rate_deg` per second: 0.3 m and 2 degrees per 0.1 s scan)."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    yaw = np.deg2rad(yaw_rate_deg) * t
    T = np.tile(np.eye(4), (len(t), 1, 1))
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    T[:, 0, 3] = speed * t
    return T


def ranges_per_ray(directions, poses):
    """SY.scene_ranges with one pose per ray: directions [3,n] (sensor frame), poses [n,4,4] -> ranges fp64 [n]"""
    d = np.einsum("nab,bn->na", poses[:, :3, :3], np.asarray(directions, dtype=np.float64))
    o = poses[:, :3, 3]
    lo, hi = np.array(SY.BOX_MIN), np.array(SY.BOX_MAX)
    safe = np.where(np.abs(d) < 1e-12, 1e-12, d)
    t_box = np.maximum((lo - o) / safe, (hi - o) / safe).min(1)
    oc = o - np.array(SY.SPHERE_C)
    b = (d * oc).sum(1)
    c = (oc * oc).sum(1) - SY.SPHERE_R ** 2
    disc = b * b - c
    t_s = np.where(disc > 0, -b - np.sqrt(np.clip(disc, 0, None)), np.inf)
    t_s = np.where(t_s > 0, t_s, np.inf)
    t = np.minimum(t_box, t_s)
    hit = o + d * t_box[:, None]
    through = (t_box <= t_s) & (hit[:, 0] > SY.BOX_MAX[0] - 1e-6) & (np.abs(hit[:, 1]) < SY.WINDOW_HALF_Y) \
        & (hit[:, 2] > SY.WINDOW_Z[0]) & (hit[:, 2] < SY.WINDOW_Z[1])
    return np.where(through, (SY.WINDOW_FAR_X - o[:, 0]) / safe[:, 0], t)


def distorted_scan(k, beams=64, azimuths=1024, period=0.1, **motion):
    """Scan k of a spinning sensor in motion: the pattern of SY.lidar_pattern in azimuth-major order (time sweeps the azimuth), ray i
    fired at k period + i period / n and cast from the pose interpolated at that time.  -> (directions [3,n] fp32, distances [n]
    fp32, timestamps [n] fp32)"""
    dirs, _ = SY.lidar_pattern(beams, azimuths)
    dirs = dirs.reshape(3, beams, azimuths).permute(0, 2, 1).reshape(3, -1).contiguous()
    n = dirs.shape[1]
    ts = (k * period + period * torch.arange(n, dtype=torch.float64) / n).float()
    r = ranges_per_ray(dirs.numpy(), pose_at(ts.double().numpy(), **motion))
    return dirs, torch.from_numpy(r).float(), ts


def surface_distance(points):
    """distance of world points [n,3] to the nearest analytic surface (box walls, the far plane behind the window, the sphere)"""
    p = np.asarray(points, dtype=np.float64)
    lo, hi = np.array(SY.BOX_MIN), np.array(SY.BOX_MAX)
    walls = np.minimum(np.abs(p - lo), np.abs(p - hi)).min(1)
    far = np.abs(p[:, 0] - SY.WINDOW_FAR_X)
    sphere = np.abs(np.linalg.norm(p - np.array(SY.SPHERE_C), axis=1) - SY.SPHERE_R)
    return np.minimum(np.minimum(walls, far), sphere)
