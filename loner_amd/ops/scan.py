"""Scan ingestion and tracking: scans from raw points, frame clouds, motion compensation, sky rays.
The tracker's per-scan calls: inputs must already be float32 (timestamps may be fp64) - a wrong dtype or shape is a ValueError,
nothing is converted silently.  scan_from_points and sky_rays read their counts back once and hold their scratch per device; the
other two read nothing back.  RuntimeError: what only the data shows."""
import ctypes as C
import math

import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _f32c, _held_buffer, _scratch


def scan_from_points(xyz, point_times, stamp, fov_segments=None, min_range=0.3, recompute_timestamps=False):
    """build_scan_from_msg on the device (include/loner_hip.h: lnr_scan_from_points).  xyz [n,3] fp32 and point_times ([n] fp32, or
    None) on the device; fov_segments None (FOV test off) or a list of at most 8 (lo, hi) degree pairs -> (ray_directions [3,M],
    distances [M], timestamps [M], order [M] int64, info): the time-ordered scan, the original index of its points, and the call's
    eight status words as Python ints.  One device -> host read (info); M == 0 and non-finite times are the caller's to refuse."""
    require_device(xyz, point_times)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32:
        raise ValueError(f"scan_from_points: xyz float32 [n,3], got {tuple(xyz.shape)} {xyz.dtype}")
    n = xyz.shape[0]
    if point_times is not None and (point_times.shape != (n,) or point_times.dtype != torch.float32):
        raise ValueError(f"scan_from_points: point_times float32 [{n}], got {tuple(point_times.shape)} {point_times.dtype}")
    segs = [] if fov_segments is None else [(float(lo), float(hi)) for lo, hi in fov_segments]
    if len(segs) > hip.SCAN_MAX_FOV_SEGMENTS:
        raise ValueError(f"scan_from_points: {len(segs)} FOV segments, at most {hip.SCAN_MAX_FOV_SEGMENTS}")
    stamp, min_range = float(stamp), float(min_range)
    if not math.isfinite(stamp) or math.isnan(min_range):
        raise ValueError(f"scan_from_points: stamp must be finite and min_range a number, got {stamp!r} and {min_range!r}")
    mode = hip.SCAN_TIME_NONE if point_times is None else hip.SCAN_TIME_RECOMPUTE if recompute_timestamps else hip.SCAN_TIME_GIVEN
    lib = load()
    dev = xyz.device
    ws, need = _scratch(lib.lnr_scan_from_points_workspace(n), dev, f"scan_from_points: {n} points, the limit per call is 2^31 - 4096",
                        held="scan")
    dirs = torch.empty(3 * n, device=dev, dtype=torch.float32)
    dist = torch.empty(n, device=dev, dtype=torch.float32)
    times = torch.empty(n, device=dev, dtype=torch.float32)
    order = torch.empty(n, device=dev, dtype=torch.int64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    flat = (C.c_float * max(2 * len(segs), 1))(*[v for s in segs for v in s])
    times_in = None if mode != hip.SCAN_TIME_GIVEN else point_times.contiguous()
    check(lib.lnr_scan_from_points(_ptr(xyz.contiguous()), _ptr(times_in), n, mode, stamp, int(fov_segments is not None), flat, len(segs), min_range,
                                   _ptr(ws), need, _ptr(dirs), _ptr(dist), _ptr(times), _ptr(order), _ptr(info), _stream()), "lnr_scan_from_points")
    info = [int(v) for v in info.cpu()]
    m = info[0]
    return dirs[:3 * m].view(3, m), dist[:m], times[:m], order[:m], info


def _scan_soa(directions, distances, what):
    require_device(directions, distances)
    if directions.dim() != 2 or directions.shape[0] != 3 or distances.dim() != 1 or distances.shape[0] != directions.shape[1]:
        raise ValueError(f"{what}: ray_directions [3,n] and distances [n], got {tuple(directions.shape)} and {tuple(distances.shape)}")
    if directions.dtype != torch.float32 or distances.dtype != torch.float32:
        raise ValueError(f"{what}: ray_directions and distances must be float32")


def frame_cloud(directions, distances, start, stop, step):
    """Frame.build_point_cloud's array (include/loner_hip.h: lnr_frame_cloud): the fp32 products dir * dist of scan entries
    start, start + step, ... below stop, widened -> points [m,3] fp64 on the scan's device."""
    _scan_soa(directions, distances, "frame_cloud")
    n = distances.shape[0]
    start, stop, step = int(start), int(stop), int(step)
    if not (0 <= start and stop <= n and step >= 1):
        raise ValueError(f"frame_cloud: bad window [{start}, {stop}) step {step} of {n} points")
    m = len(range(start, stop, step))
    points = torch.empty(m, 3, device=distances.device, dtype=torch.float64)
    check(load().lnr_frame_cloud(_ptr(_f32c(directions)), _ptr(_f32c(distances)), n, start, stop, step, _ptr(points), _stream()), "lnr_frame_cloud")
    return points


def motion_compensate(directions, distances, timestamps, t0, denom, consts):
    """LidarScan.motion_compensate in place on directions [3,n] and distances [n] (include/loner_hip.h: lnr_motion_compensate).
    timestamps [n] fp32 or fp64; t0 and denom = t1 - t0 as floats; consts: the LNR_MOCOMP_CONSTS fp64 per-call constants."""
    _scan_soa(directions, distances, "motion_compensate")
    require_device(timestamps)
    n = distances.shape[0]
    if timestamps.shape != (n,) or timestamps.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"motion_compensate: timestamps [n] float32 or float64, got {tuple(timestamps.shape)} {timestamps.dtype}")
    if not (directions.is_contiguous() and distances.is_contiguous()):
        raise ValueError("motion_compensate: works in place, ray_directions and distances must be contiguous")
    consts = [float(x) for x in consts]
    if len(consts) != hip.MOCOMP_CONSTS:
        raise ValueError(f"motion_compensate: {hip.MOCOMP_CONSTS} constants, got {len(consts)}")
    if not all(math.isfinite(x) for x in consts + [float(t0), float(denom)]):
        raise ValueError("motion_compensate: a pose or a pose time is not finite")
    c = (C.c_double * hip.MOCOMP_CONSTS)(*consts)
    check(load().lnr_motion_compensate(_ptr(directions), _ptr(distances), _ptr(timestamps.contiguous()), int(timestamps.dtype == torch.float64), n,
                                       float(t0), float(denom), c, _stream()), "lnr_motion_compensate")


def sky_rays(directions, rotation):
    """Tracker.compute_sky_rays (include/loner_hip.h: lnr_sky_rays): sensor-frame directions [3,n] fp32 and the pose's rotation [3,3]
    -> the sky directions [3,m] fp32 (rotated, in row-major pixel order).  One device -> host read (m)."""
    require_device(directions, rotation)
    if directions.dim() != 2 or directions.shape[0] != 3 or directions.shape[1] == 0 or directions.dtype != torch.float32:
        raise ValueError(f"sky_rays: ray_directions float32 [3,n] with n >= 1, got {tuple(directions.shape)} {directions.dtype}")
    dev = directions.device
    rot = rotation.detach().to(device=dev, dtype=torch.float32).contiguous()
    if rot.shape != (3, 3):
        raise ValueError(f"sky_rays: rotation [3,3], got {tuple(rot.shape)}")
    lib = load()                                # the workspace and the full-size output are kept per device; the result is copied out
    ws, need = _scratch(lib.lnr_sky_rays_workspace(), dev, held="sky")
    sky = _held_buffer("sky output", dev, 3 * hip.SKY_MAX_RAYS, torch.float32).view(3, hip.SKY_MAX_RAYS)
    info = torch.empty(8, device=dev, dtype=torch.int32)
    check(lib.lnr_sky_rays(_ptr(_f32c(directions)), directions.shape[1], _ptr(rot), _ptr(ws), need, _ptr(sky), hip.SKY_MAX_RAYS, _ptr(info),
                           _stream()), "lnr_sky_rays")
    info = [int(x) for x in info.cpu()]
    if info[0]:
        raise RuntimeError(f"sky_rays: {info[6]} ray directions are not finite")
    return sky[:, :info[1]].contiguous()
