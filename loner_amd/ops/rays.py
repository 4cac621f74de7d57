"""Rays of the mapping loop: lidar, camera and window rays, poses, compaction, the sharded loop's front record, the ray gradient.
Mapping loop, every iteration: fp32 device tensors (indices int64), outputs allocated uninitialised and written in full by the
kernel, never a read back.  Wrong dtypes or shapes are assertions; RuntimeError: a tensor is not on the device, or the library refused."""
import ctypes as C

import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _U64, _f32c, _float3


def build_lidar_rays(directions, distances, index, transform12, ray_range, scale, shift):
    """-> (rays [m,13], depths [m], keep [m] uint8) for ALL candidates."""
    require_device(directions, distances, index, transform12)
    directions, distances, transform12 = _f32c(directions), _f32c(distances), _f32c(transform12)
    index = index.to(torch.int64).contiguous()
    m = index.shape[0]
    dev = directions.device
    rays = torch.empty(m, hip.RAY_STRIDE, device=dev, dtype=torch.float32)
    depths = torch.empty(m, device=dev, dtype=torch.float32)
    keep = torch.empty(m, device=dev, dtype=torch.uint8)
    check(load().lnr_build_lidar_rays(_ptr(directions), _ptr(distances), directions.shape[1], _ptr(index), m, _ptr(transform12), float(ray_range[0]),
                                      float(ray_range[1]), float(scale), _float3(shift), _ptr(rays), _ptr(depths), _ptr(keep),
                                      _stream()), "lnr_build_lidar_rays")
    return rays, depths, keep


def build_camera_rays(directions, index, width, transform12, range_min, scale, shift):
    """-> rays [n,13] of a pinhole image (lnr_build_camera_rays).  directions [n_pixels,3] fp32 on the device; index: int64 pixel
    indices on the device, or None for every pixel in order."""
    require_device(directions, index, transform12)
    directions, transform12 = _f32c(directions), _f32c(transform12)
    assert directions.dim() == 2 and directions.shape[1] == 3 and transform12.numel() == 12
    n_pixels = directions.shape[0]
    if index is not None:
        index = index.to(torch.int64).contiguous()
    n = n_pixels if index is None else index.shape[0]
    rays = torch.empty(n, hip.RAY_STRIDE, device=directions.device, dtype=torch.float32)
    check(load().lnr_build_camera_rays(_ptr(directions), n_pixels, _ptr(index), n, int(width), _ptr(transform12), float(range_min), float(scale),
                                       _float3(shift), _ptr(rays), _stream()), "lnr_build_camera_rays")
    return rays


class WindowTables:
    """Host-side per-segment tables of a keyframe window for lnr_build_window_rays (built once per window)."""

    def __init__(self, dirs_list, dist_list, const_dist, seg_counts, seg_pose):
        n = len(dirs_list)
        self.n_seg = n
        self.keepalive = (list(dirs_list), list(dist_list))
        self.dirs = (C.c_void_p * n)(*[d.data_ptr() for d in dirs_list])
        self.dist = (C.c_void_p * n)(*[(d.data_ptr() if d is not None else None) for d in dist_list])
        self.const_dist = (C.c_float * n)(*[float(c) for c in const_dist])
        self.n_points = (C.c_int64 * n)(*[int(d.shape[1]) for d in dirs_list])
        starts = [0]
        for c in seg_counts:
            starts.append(starts[-1] + int(c))
        self.seg_start_list = starts
        self.seg_start = (C.c_int32 * (n + 1))(*starts)
        self.seg_pose = (C.c_int32 * n)(*[int(p) for p in seg_pose])
        self.total = starts[-1]


def build_window_rays(tab: WindowTables, transforms, ray_range, scale, shift, index=None, seed=0):
    """-> (rays [total,13], depths, keep, src_index) for every candidate of the window, one launch."""
    require_device(transforms, index)
    dev = transforms.device
    rays = torch.empty(tab.total, hip.RAY_STRIDE, device=dev, dtype=torch.float32)
    depths = torch.empty(tab.total, device=dev, dtype=torch.float32)
    keep = torch.empty(tab.total, device=dev, dtype=torch.uint8)
    idx_out = None
    if index is None:
        idx_out = torch.empty(tab.total, device=dev, dtype=torch.int64)
    else:
        index = index.to(torch.int64).contiguous()
    check(load().lnr_build_window_rays(tab.dirs, tab.dist, tab.const_dist, tab.n_points, tab.seg_start, tab.seg_pose, tab.n_seg, _ptr(index), _ptr(idx_out),
                                       int(seed) & _U64, _ptr(_f32c(transforms)), float(ray_range[0]), float(ray_range[1]), float(scale), _float3(shift),
                                       _ptr(rays), _ptr(depths), _ptr(keep), _stream()), "lnr_build_window_rays")
    return rays, depths, keep, (index if index is not None else idx_out)


def pose_forward(pose6):
    require_device(pose6)
    p = _f32c(pose6.detach()).reshape(-1, 6)
    T = torch.empty(p.shape[0], 12, device=p.device, dtype=torch.float32)
    if p.shape[0] == 0:                   # (an empty tensor has no address to hand over)
        return T
    check(load().lnr_pose_forward(_ptr(p), p.shape[0], _ptr(T), _stream()), "lnr_pose_forward")
    return T


def pose_backward(pose6, d_transforms, mask=None, out=None, accumulate=False, poison=None, poison_tag=0):
    """poison (int32[2] device word, optional): failure guard, see include/loner_hip.h."""
    require_device(pose6, d_transforms, mask, out, poison)
    p = _f32c(pose6.detach()).reshape(-1, 6)
    if out is None:
        out = torch.empty_like(p)
        accumulate = False
    if p.shape[0] == 0:
        return out
    check(load().lnr_pose_backward(_ptr(p), _ptr(_f32c(d_transforms)), _ptr(mask), p.shape[0], _ptr(out), int(accumulate), _ptr(poison), int(poison_tag),
                                   _stream()), "lnr_pose_backward")
    return out


def compact_rays(rays, depths, keep, src_index, seg_start, n_out=None, want_counts=False, front=None):
    """seg_start: python list [n_seg+1] (or the ctypes int32 array of a WindowTables).  -> (rays_out [cap,13], depths_out, src_out, out_seg_start dev int32
    [n_seg+1], n_out dev int32 [1]); only the first n_out rows are meaningful.  n_out (optional): an int32 [1] device tensor the
    live count is written into (the training loop hands in a row of its per-iteration log instead of copying into it afterwards).
    want_counts / front = (seg_order ctypes array or list, cap): the same launch also computes count_opaque's {#rays, #opaque rays} /
    writes the rank's front record (shard_front_pack) - a sixth return value, counts int32 [2] or record float32 [FRONT_HEADER + cap]."""
    require_device(rays, depths, keep, src_index)
    n_in, dev = rays.shape[0], rays.device
    n_seg = len(seg_start) - 1
    rays_out = torch.empty_like(rays)
    depths_out = torch.empty_like(depths)
    src_out = torch.empty_like(src_index) if src_index is not None else None
    # (both are written in full by the kernel: no fill launches - the front end of an iteration is a chain of small kernels)
    out_seg = torch.empty(n_seg + 1, device=dev, dtype=torch.int32)
    if n_out is None:
        n_out = torch.empty(1, device=dev, dtype=torch.int32)
    else:
        require_device(n_out)
        assert n_out.dtype == torch.int32 and n_out.numel() == 1 and n_out.is_contiguous()
    seg = seg_start if isinstance(seg_start, C.Array) else (C.c_int32 * (n_seg + 1))(*[int(v) for v in seg_start])
    if want_counts or front is not None:
        counts = rec = order = None
        cap = 0
        if front is not None:
            order, cap = front
            if not isinstance(order, C.Array):
                order = (C.c_int32 * n_seg)(*[int(v) for v in order])
            rec = torch.empty(hip.FRONT_HEADER + int(cap), device=dev, dtype=torch.float32)
        else:
            counts = torch.empty(2, device=dev, dtype=torch.int32)
        check(load().lnr_compact_rays_front(_ptr(rays), _ptr(depths), _ptr(keep), _ptr(src_index), n_in, seg, n_seg, _ptr(rays_out), _ptr(depths_out),
                                            _ptr(src_out), _ptr(out_seg), _ptr(n_out), _ptr(counts), order, int(cap), _ptr(rec),
                                            _stream()), "lnr_compact_rays_front")
        return rays_out, depths_out, src_out, out_seg, n_out, (rec if front is not None else counts)
    check(load().lnr_compact_rays(_ptr(rays), _ptr(depths), _ptr(keep), _ptr(src_index), n_in, seg, n_seg, _ptr(rays_out), _ptr(depths_out), _ptr(src_out),
                                  _ptr(out_seg), _ptr(n_out), _stream()), "lnr_compact_rays")
    return rays_out, depths_out, src_out, out_seg, n_out


def first_ray_key(rays, out_seg_start, seg_order):
    """int64 [1] on the device: (window order of this rank's first segment with a kept ray) << 32 | float bits of that ray's far,
    INT64_MAX without one (mapping/sharding.py: the far[0] of a sharded batch)."""
    require_device(rays, out_seg_start)
    n_seg = len(seg_order)
    key = torch.empty(1, device=rays.device, dtype=torch.int64)
    order = (C.c_int32 * n_seg)(*[int(v) for v in seg_order])
    check(load().lnr_first_ray_key(_ptr(rays), _ptr(out_seg_start), order, n_seg, _ptr(key), _stream()), "lnr_first_ray_key")
    return key


def shard_front_pack(rays, out_seg_start, seg_order, depths, n_rays_dev, cap, device=None):
    """A rank's "front record" for the sharded loop's one all-gather (include/loner_hip.h: lnr_shard_front_pack): float32
    [FRONT_HEADER + cap] = first-ray key | live-ray count | ground-truth depths.  rays None: a rank without keyframes."""
    dev = rays.device if rays is not None else torch.device(device)
    rec = torch.empty(hip.FRONT_HEADER + int(cap), device=dev, dtype=torch.float32)
    if rays is None:
        check(load().lnr_shard_front_pack(None, None, None, 0, None, 0, None, int(cap), _ptr(rec), _stream()), "lnr_shard_front_pack")
        return rec
    require_device(rays, out_seg_start, depths, n_rays_dev)
    n_seg = len(seg_order)
    order = seg_order if isinstance(seg_order, C.Array) else (C.c_int32 * n_seg)(*[int(v) for v in seg_order])
    check(load().lnr_shard_front_pack(_ptr(rays), _ptr(out_seg_start), order, n_seg, _ptr(_f32c(depths)), rays.shape[0], _ptr(n_rays_dev), int(cap),
                                      _ptr(rec), _stream()), "lnr_shard_front_pack")
    return rec


def shard_front_reduce(records, world, stride):
    """gathered front records [world * stride] -> (counts int32 [2] = {#rays, #opaque rays} of the WHOLE batch, far0 float [1])"""
    require_device(records)
    assert records.dtype == torch.float32 and records.numel() == world * stride
    counts = torch.empty(2, device=records.device, dtype=torch.int32)
    far0 = torch.empty(1, device=records.device, dtype=torch.float32)
    check(load().lnr_shard_front_reduce(_ptr(records), int(world), int(stride), _ptr(counts), _ptr(far0), _stream()), "lnr_shard_front_reduce")
    return counts, far0


def lidar_rays_backward(d_rays, rays, src_index, seg_start_dev, directions_list, transforms, scale):
    """-> d_transform [n_seg, 12]"""
    require_device(d_rays, rays, src_index, seg_start_dev, transforms)
    n_seg = len(directions_list)
    dev = rays.device
    out = torch.empty(n_seg, 12, device=dev, dtype=torch.float32) if rays.shape[0] > 0 else torch.zeros(n_seg, 12, device=dev)
    ptrs = (C.c_void_p * n_seg)(*[d.data_ptr() for d in directions_list])
    npts = (C.c_int64 * n_seg)(*[int(d.shape[1]) for d in directions_list])
    check(load().lnr_lidar_rays_backward(_ptr(_f32c(d_rays)), _ptr(rays), _ptr(src_index), _ptr(seg_start_dev), n_seg, ptrs, npts, _ptr(_f32c(transforms)),
                                         float(scale), _ptr(out), _stream()), "lnr_lidar_rays_backward")
    return out
