"""Rays [n,6] against geometry: the BVH over a triangle mesh with its ray casts, closest points and crossing counts, the rays of a
moving sensor, and the TSDF volume that rays are fused into.
Offline tools: rays, points and ranges of a float dtype are widened to fp64.  The BVH build reads its status back once; a walk reads
back only for a caller who hands in a `stats` dict, and only then raises on a status bit; the TSDF calls read nothing back.
ValueError: an argument the caller got wrong, refused before a launch.  RuntimeError: what only the data shows."""
import ctypes as C
import math

import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _f64_points, _float_rows, _mesh_triangles, _positive, _raise_status, _scratch
from .cloud import Trajectory

_BVH_STATUS = {1: "a vertex index is out of range", 2: "the tree is deeper than the traversal stack"}
_CAST_STATUS = {**_BVH_STATUS, 4: "a ray reached the visit cap", 8: "a traversal stack was full"}


class BVH:
    """The device BVH over a triangle mesh (include/loner_hip.h: lnr_bvh_build), reusable for any number of ray batches: vertices
    [V,3] (fp64) and triangles [F,3] int32 on the device.  The buffer holds its own copy of the corners.  .n_triangles (F),
    .n_in_tree, .n_nonfinite (triangles left out for a non-finite vertex), .depth, .n_nodes: what the build reports (one host read).
    Raises RuntimeError on a vertex index out of range."""

    def __init__(self, vertices, triangles):
        v = _f64_points(vertices, "BVH")
        tri = _mesh_triangles(triangles, "BVH")
        if tri.device != v.device:
            raise ValueError(f"BVH: vertices on {v.device}, triangles on {tri.device}")
        f, dev = tri.shape[0], v.device
        lib = load()
        over_limit = f"BVH: {f} triangles, the limit is 2^31 - 4096"
        self.n_triangles = f
        self.buf, nbytes = _scratch(lib.lnr_bvh_bytes(f), dev, over_limit)
        ws, need = _scratch(lib.lnr_bvh_workspace(f), dev, over_limit)
        info = torch.empty(hip.RAYCAST_INFO, device=dev, dtype=torch.int64)
        check(lib.lnr_bvh_build(_ptr(v), v.shape[0], _ptr(tri), f, _ptr(ws), need, _ptr(self.buf), nbytes, _ptr(info), _stream()), "lnr_bvh_build")
        host = info.cpu()
        _raise_status("BVH", int(host[0]), _BVH_STATUS, f"{int(host[3])} triangles with an index out of range: ")
        self.n_in_tree, self.n_nonfinite, self.depth, self.n_nodes = int(host[1]), int(host[2]), int(host[4]), int(host[5])

    @property
    def device(self):
        return self.buf.device


def _walk_input(bvh, t, what, name):
    """the rays or points of a walk, checked to lie on the BVH's device, as contiguous fp64"""
    if t.device != bvh.device:
        raise ValueError(f"{what}: {name} on {t.device}, the BVH on {bvh.device}")
    require_device(t)
    return t.to(torch.float64).contiguous()


def _window(what, t_min, t_max):
    lo, hi = float(t_min), float(t_max)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f"{what}: t_min and t_max must be numbers, got {t_min!r} and {t_max!r}")
    return lo, hi


def _require_bvh(what, bvh, t=None, width=0, name=""):
    if not isinstance(bvh, BVH):
        raise ValueError(f"{what}: bvh must be an ops.BVH, got {type(bvh).__name__}")
    if width:
        _float_rows(t, width, what, name)


def _walk(what, device, call, stats, names):
    """A BVH walk, call(info pointer) checked as lnr_<what>; with a stats dict, its one host read: raise on a status bit, else fill stats"""
    info = torch.empty(hip.RAYCAST_INFO, device=device, dtype=torch.int64)
    check(call(_ptr(info)), "lnr_" + what)
    if stats is not None:
        host = info.cpu()
        _raise_status(what, int(host[0]), _CAST_STATUS)
        stats.update({name: int(host[1 + i]) for i, name in enumerate(names)})


def cast_rays(bvh, rays, t_min=0.0, t_max=math.inf, want_uvs=True, stats=None):
    """open3d's RaycastingScene.cast_rays with a window (include/loner_hip.h: lnr_cast_rays): rays [n,6] (ox oy oz dx dy dz) on the
    BVH's device -> (t_hit fp64 [n], +inf on a miss; primitive_ids int32 [n], -1 on a miss; primitive_uvs fp64 [n,2] or None).
    stats (a dict, optional) receives {"hits", "invalid_rays", "node_visits", "capped_rays", "excluded_triangles", "depth"} at the
    price of one device -> host read, which then also raises RuntimeError on a status bit; without it nothing is read back."""
    _require_bvh("cast_rays", bvh)
    require_device(rays)
    if rays.dim() != 2 or rays.shape[1] != 6:          # (any dtype: this call's own, older check and text)
        raise ValueError(f"cast_rays: rays [n,6], got {tuple(rays.shape)}")
    lo, hi = _window("cast_rays", t_min, t_max)
    r = _walk_input(bvh, rays, "cast_rays", "rays")
    n, dev = r.shape[0], r.device
    t_hit = torch.empty(n, device=dev, dtype=torch.float64)
    ids = torch.empty(n, device=dev, dtype=torch.int32)
    uvs = torch.empty(n, 2, device=dev, dtype=torch.float64) if want_uvs else None
    _walk("cast_rays", dev, lambda info: load().lnr_cast_rays(_ptr(bvh.buf), bvh.n_triangles, _ptr(r), n, lo, hi, _ptr(t_hit), _ptr(ids),
                                                               _ptr(uvs), info, _stream()),
          stats, ("hits", "invalid_rays", "node_visits", "capped_rays", "excluded_triangles", "depth"))
    return t_hit, ids, uvs


def closest_points(bvh, points, max_distance=math.inf, want_points=True, want_uvs=True, stats=None):
    """open3d's RaycastingScene.compute_closest_points with a reach (include/loner_hip.h: lnr_closest_points): points [n,3] (a float
    dtype) on the BVH's device -> (dist_sq fp64 [n], +inf with no triangle within max_distance; primitive_ids int32 [n], -1 then;
    closest fp64 [n,3] or None; primitive_uvs fp64 [n,2] or None).  stats (a dict, optional) receives {"answered", "invalid_points",
    "node_visits", "capped", "excluded_triangles", "depth"} at the price of one device -> host read, which then also raises
    RuntimeError on a status bit; without it nothing is read back."""
    _require_bvh("closest_points", bvh, points, 3, "points")
    reach = float(max_distance)
    if math.isnan(reach) or reach < 0:
        raise ValueError(f"closest_points: max_distance must be a number >= 0, got {max_distance!r}")
    p = _walk_input(bvh, points, "closest_points", "points")
    n, dev = p.shape[0], p.device
    dist_sq = torch.empty(n, device=dev, dtype=torch.float64)
    ids = torch.empty(n, device=dev, dtype=torch.int32)
    closest = torch.empty(n, 3, device=dev, dtype=torch.float64) if want_points else None
    uvs = torch.empty(n, 2, device=dev, dtype=torch.float64) if want_uvs else None
    _walk("closest_points", dev, lambda info: load().lnr_closest_points(_ptr(bvh.buf), bvh.n_triangles, _ptr(p), n, reach * reach,
                                                                         _ptr(dist_sq), _ptr(ids), _ptr(closest), _ptr(uvs), info, _stream()),
          stats, ("answered", "invalid_points", "node_visits", "capped", "excluded_triangles", "depth"))
    return dist_sq, ids, closest, uvs


def count_intersections(bvh, rays, t_min=0.0, t_max=math.inf, stats=None):
    """open3d's RaycastingScene.count_intersections with a window (include/loner_hip.h: lnr_count_intersections): rays [n,6] (a float
    dtype) on the BVH's device -> counts int32 [n], the triangles each ray crosses with t_min <= t <= t_max.  stats (a dict,
    optional) receives {"rays_crossing", "invalid_rays", "node_visits", "capped", "excluded_triangles", "depth"} at the price of one
    device -> host read, which then also raises RuntimeError on a status bit."""
    _require_bvh("count_intersections", bvh, rays, 6, "rays")
    lo, hi = _window("count_intersections", t_min, t_max)
    r = _walk_input(bvh, rays, "count_intersections", "rays")
    n, dev = r.shape[0], r.device
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    _walk("count_intersections", dev, lambda info: load().lnr_count_intersections(_ptr(bvh.buf), bvh.n_triangles, _ptr(r), n, lo, hi,
                                                                                   _ptr(counts), info, _stream()),
          stats, ("rays_crossing", "invalid_rays", "node_visits", "capped", "excluded_triangles", "depth"))
    return counts


def trajectory_rays(directions, timestamps, trajectory):
    """The rays of a sensor that moves while it sweeps (include/loner_hip.h: lnr_trajectory_rays): directions [3,n] fp32 in the sensor
    frame, timestamps [n] (absolute, widened to fp64), trajectory a Trajectory on the same device -> (rays fp64 [n,6], NaN where the
    time lies outside the trajectory or an input is not finite; info int64 [8] on the device: {status, rays, outside, non-finite})."""
    require_device(directions, timestamps)
    if directions.dim() != 2 or directions.shape[0] != 3 or directions.dtype != torch.float32:
        raise ValueError(f"trajectory_rays: directions fp32 [3,n], got {tuple(directions.shape)} {directions.dtype}")
    n = directions.shape[1]
    if tuple(timestamps.shape) != (n,):
        raise ValueError(f"trajectory_rays: timestamps [{n}], got {tuple(timestamps.shape)}")
    if not isinstance(trajectory, Trajectory):
        raise ValueError(f"trajectory_rays: trajectory must be an ops.Trajectory, got {type(trajectory).__name__}")
    d = directions.contiguous()
    stamps = timestamps.to(torch.float64).contiguous()
    dev = d.device
    rays = torch.empty(n, 6, device=dev, dtype=torch.float64)
    info = torch.empty(hip.RAYCAST_INFO, device=dev, dtype=torch.int64)
    tr = trajectory
    check(load().lnr_trajectory_rays(_ptr(d), _ptr(stamps), n, _ptr(tr.times), _ptr(tr.positions), _ptr(tr.rotations), _ptr(tr.rotvecs), tr.n_poses,
                                     _ptr(rays), _ptr(info), _stream()), "lnr_trajectory_rays")
    return rays, info


def _tsdf_volume(sum_, count, what):
    """the checks the two TSDF calls share -> (nx, ny, nz)"""
    require_device(sum_, count)
    if sum_.dim() != 3 or sum_.dtype != torch.int64 or count.dtype != torch.uint32 or count.shape != sum_.shape or count.device != sum_.device:
        raise ValueError(f"{what}: sum int64 [nx,ny,nz] and count uint32 of the same shape on one device, got {sum_.dtype} "
                         f"{tuple(sum_.shape)} and {count.dtype} {tuple(count.shape)}")
    nx, ny, nz = (int(x) for x in sum_.shape)
    if min(nx, ny, nz) < 2 or nx * ny * nz >= 1 << 31:
        raise ValueError(f"{what}: every axis needs at least two nodes and the volume fewer than 2^31, got {nx} x {ny} x {nz}")
    return nx, ny, nz


def tsdf_integrate(rays, ranges, sum_, count, origin, voxel_size, trunc, front=None):
    """Adds rays to a TSDF volume in place (include/loner_hip.h: lnr_tsdf_integrate): rays [n,6] (ox oy oz dx dy dz, unit directions)
    and ranges [n] of a float dtype, sum_ int64 [nx,ny,nz] and count uint32 [nx,ny,nz] (zeroed by the caller before the first call),
    all on one device; node (i,j,k) lies at origin + (i,j,k) * voxel_size.  front (default: trunc) is how far in front of the return a
    ray writes; math.inf carves free space from the sensor on.  -> info int64 [8] on the device: {status, rays that updated a node,
    invalid rays, rays that miss the volume, node updates}."""
    nx, ny, nz = _tsdf_volume(sum_, count, "tsdf_integrate")
    require_device(rays, ranges)
    _float_rows(rays, 6, "tsdf_integrate", "rays")
    n = rays.shape[0]
    if tuple(ranges.shape) != (n,) or not ranges.dtype.is_floating_point:
        raise ValueError(f"tsdf_integrate: ranges [{n}] of a float dtype, got {tuple(ranges.shape)} {ranges.dtype}")
    if rays.device != sum_.device or ranges.device != sum_.device:
        raise ValueError(f"tsdf_integrate: rays on {rays.device}, ranges on {ranges.device}, the volume on {sum_.device}")
    org = [float(x) for x in origin]
    if len(org) != 3 or not all(math.isfinite(x) for x in org):
        raise ValueError(f"tsdf_integrate: origin must be three finite numbers, got {origin!r}")
    v, tr = _positive(voxel_size, "tsdf_integrate", "voxel_size"), _positive(trunc, "tsdf_integrate", "trunc")
    fr = tr if front is None else float(front)
    if not fr >= tr:
        raise ValueError(f"tsdf_integrate: front must be at least trunc ({tr}), got {front!r}")
    r = rays.to(torch.float64).contiguous()
    rng = ranges.to(torch.float64).contiguous()
    info = torch.empty(8, device=sum_.device, dtype=torch.int64)
    check(load().lnr_tsdf_integrate(_ptr(r), _ptr(rng), n, nx, ny, nz, (C.c_double * 3)(*org), v, tr, fr, _ptr(sum_), _ptr(count), _ptr(info),
                                    _stream()), "lnr_tsdf_integrate")
    return info


def tsdf_field(sum_, count, min_count=1):
    """A TSDF volume's mean (include/loner_hip.h: lnr_tsdf_field) -> (field fp32 [nx,ny,nz]: minus the mean truncated distance in units
    of trunc, > 0 behind the surface, 0 where nothing was observed; valid uint8 [nx,ny,nz]: count >= min_count), on the device."""
    nx, ny, nz = _tsdf_volume(sum_, count, "tsdf_field")
    if isinstance(min_count, bool) or int(min_count) != min_count or not 1 <= min_count < 1 << 32:
        raise ValueError(f"tsdf_field: min_count must be an integer in [1, 2^32), got {min_count!r}")
    field = torch.empty(nx, ny, nz, device=sum_.device, dtype=torch.float32)
    valid = torch.empty(nx, ny, nz, device=sum_.device, dtype=torch.uint8)
    check(load().lnr_tsdf_field(_ptr(sum_), _ptr(count), nx, ny, nz, int(min_count), _ptr(field), _ptr(valid), _stream()), "lnr_tsdf_field")
    return field, valid
