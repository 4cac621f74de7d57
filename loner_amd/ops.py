"""Tensor-level wrappers around the C ABI (one Python function per entry point).

Every function takes/returns torch tensors that live on the HIP device, allocates outputs with
torch, and enqueues the kernel on torch's current stream.  No function here computes anything
itself - the arithmetic is in libloner_hip.so.
"""
import ctypes as C
import math
import os

import torch

from . import hip
from .hip import _ptr, _stream, check, load, require_device

_steps_cache = {}


def linspace_table(count: int, device) -> torch.Tensor:
    """torch.linspace(0,1,count) on `device` (ray_sampling.py:27,59); cached."""
    key = (count, str(device))
    t = _steps_cache.get(key)
    if t is None:
        t = torch.linspace(0, 1, count).to(device)
        _steps_cache[key] = t
    return t


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# ---------------------------------------------------------------- diagnostics
def profile_enable(on=True):
    """Per-kernel HIP-event timing inside lnr_density_forward / lnr_density_backward (off by default)."""
    check(load().lnr_profile_enable(1 if on else 0), "lnr_profile_enable")


def profile_read():
    """-> {kernel: {"calls": n, "total_ms": t, "avg_ms": t / n}}; waits for the recorded events and clears the log."""
    cap, stride = 64, 48
    names = C.create_string_buffer(cap * stride)
    ms = (C.c_float * cap)()
    calls = (C.c_int32 * cap)()
    n = load().lnr_profile_read(names, stride, ms, calls, cap)
    out = {}
    for i in range(max(n, 0)):
        name = names.raw[i * stride:(i + 1) * stride].split(b"\0", 1)[0].decode()
        out[name] = {"calls": int(calls[i]), "total_ms": float(ms[i]), "avg_ms": float(ms[i]) / max(int(calls[i]), 1)}
    return out


# ---------------------------------------------------------------- density network
_workspaces = {}
_BINS_W8 = bool(os.environ.get("LNR_BINS_W8"))
_BINS = bool(os.environ.get("LNR_BINS"))            # A/B switch of the experiment scripts (tools/): the binned partition on hashed levels


def _workspace(spec, device, n_points, forward_only=False):
    """One scratch buffer per device, grown on demand (feature planes, gradient records, ... - see the header).
    forward_only: sized for lnr_density_forward alone (no backward will follow on these points)."""
    lib = load()
    need = (lib.lnr_density_workspace_forward if forward_only else lib.lnr_density_workspace)(C.byref(spec), int(n_points))
    key = str(device)
    ent = _workspaces.get(key)
    if ent is None or ent["buf"].numel() * 4 < need:
        clipped = 0 if ent is None else ent["clipped_before"] + int(ent["buf"][:1].view(torch.int32).item())
        if ent is not None:                         # the library's note about the old buffer goes with it (include/loner_hip.h)
            check(load().lnr_density_workspace_release(_ptr(ent["buf"])), "lnr_density_workspace_release")
        _workspaces.pop(key, None)
        ent = None                                  # release the old buffer before the larger one is allocated
        ent = {"buf": torch.empty((need + 3) // 4, device=device, dtype=torch.float32), "features_of": None, "clipped_before": clipped}
        check(load().lnr_density_workspace_init(_ptr(ent["buf"]), ent["buf"].numel() * 4, _stream()), "lnr_density_workspace_init")
        _workspaces[key] = ent
    return ent, need


def density_route(spec, n_points, backward=True):
    """-> hip.DensityRoute: the MLP kernels the library launches for `spec` at `n_points` points (`kind` indexes hip.ROUTE_KINDS).  No GPU."""
    r = hip.DensityRoute()
    check(load().lnr_density_route(C.byref(spec), int(n_points), 1 if backward else 0, C.byref(r)), "lnr_density_route")
    return r


def density_clipped_count(device) -> int:
    """Number of density outputs the forward kernels have clipped on `device` so far (non-finite values, and values beyond
    +-65504 in the fp16 mode: nerf_tcnn.py:70-78).  Reads a status word of the workspace: synchronises with the device."""
    ent = _workspaces.get(str(device))
    if ent is None:
        return 0
    return ent["clipped_before"] + int(ent["buf"][hip.STATUS_CLIPPED:hip.STATUS_CLIPPED + 1].view(torch.int32).item())


def _sigma_out(out, shape, device):
    if out is None:
        return torch.empty(*shape, device=device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(shape) and out.device == device
    return out


def density_forward(spec, params, pts=None, rays=None, z=None, n_rays_dev=None, forward_only=False, out=None):
    """forward_only: the caller will not call density_backward(reuse_features=True) on these points - the workspace is sized
    for the forward alone (rendering / inference: no record regions).
    out: a contiguous float32 tensor of the result's shape to write sigma into instead of a new one (rays form: the rows from
    *n_rays_dev on keep what they held)."""
    require_device(params, pts, rays, z)
    params = _f32c(params)
    if pts is not None:
        pts = _f32c(pts).reshape(-1, 3)
        n = pts.shape[0]
        ent, need = _workspace(spec, params.device, n, forward_only)
        sigma = _sigma_out(out, (n,), params.device)
        check(load().lnr_density_forward(C.byref(spec), _ptr(params), _ptr(pts), n, None, None, 0, 0, None,
                                         _ptr(sigma), _ptr(ent["buf"]), need, _stream()), "lnr_density_forward")
        ent["features_of"] = None if forward_only else (params.data_ptr(), pts.data_ptr(), 0, n)
        return sigma
    rays, z = _f32c(rays), _f32c(z)
    n, s = z.shape
    ent, need = _workspace(spec, params.device, n * s, forward_only)
    sigma = _sigma_out(out, (n, s), params.device)      # rows >= *n_rays_dev are never read
    check(load().lnr_density_forward(C.byref(spec), _ptr(params), None, 0, _ptr(rays), _ptr(z), n, s,
                                     _ptr(n_rays_dev), _ptr(sigma), _ptr(ent["buf"]), need, _stream()), "lnr_density_forward")
    ent["features_of"] = None if forward_only else (params.data_ptr(), rays.data_ptr(), z.data_ptr(), n * s)
    return sigma


def _event(ev):
    """raw hipEvent_t of a torch.cuda.Event that has been recorded at least once (torch creates the handle lazily), or NULL"""
    if ev is None:
        return None
    h = ev.cuda_event
    if not h:
        raise RuntimeError("loner_amd: the torch event has no handle yet - record it once before handing it to the library")
    return C.c_void_p(h)


def density_backward(spec, params, d_sigma, grad_params, pts=None, rays=None, z=None, n_rays_dev=None,
                     want_d_pts=False, reuse_features=False, d_rays=None, table_atomics=False, report_regions=False, bins=False, bins_w8=False, input_grad_event=None,
                     defer_weight_fold=False, overwrite_grad=False):
    """Accumulates into grad_params [n_params] (None: parameters frozen, only the input gradient is computed);
    returns d_pts ([...,3]) or None.  table_atomics: test hook (LNR_BWD_TABLE_ATOMICS).
    reuse_features: the caller asserts that the last density_forward on this device ran on the same params and
    points (and that neither changed since), so the encoded features still in the workspace are reused.
    d_rays [n_rays,13] (rays form, instead of want_d_pts): the point gradient is reduced per ray and added to it.
    overwrite_grad: grad_params receives this call's gradient instead of accumulating it (LNR_BWD_OVERWRITE_GRAD)."""
    assert not (want_d_pts and d_rays is not None)
    require_device(params, d_sigma, grad_params, pts, rays, z)
    params, d_sigma = _f32c(params), _f32c(d_sigma)
    assert grad_params is None or (grad_params.dtype == torch.float32 and grad_params.is_contiguous())
    flags = (hip.BWD_TABLE_ATOMICS if table_atomics else 0) | (hip.BWD_REPORT_REGIONS if report_regions else 0) | \
        (hip.BWD_BINS if (bins or _BINS) else 0) | (hip.BWD_BINS_W8 if (bins_w8 or _BINS_W8) else 0) | \
        (hip.BWD_DEFER_WEIGHT_FOLD if defer_weight_fold else 0) | (hip.BWD_OVERWRITE_GRAD if overwrite_grad else 0)
    n_points = (pts.numel() // 3) if pts is not None else z.numel()
    ent, need = _workspace(spec, params.device, n_points)
    if pts is not None:
        pts = _f32c(pts).reshape(-1, 3)
        n = pts.shape[0]
        reuse = int(bool(reuse_features))
        if reuse and ent["features_of"] != (params.data_ptr(), pts.data_ptr(), 0, n):
            raise RuntimeError("density_backward(reuse_features=True): workspace features belong to a different forward call")
        d_pts = torch.empty(n, 3, device=params.device, dtype=torch.float32) if want_d_pts else None
        check(load().lnr_density_backward(C.byref(spec), _ptr(params), _ptr(pts), n, None, None, 0, 0, None,
                                          _ptr(d_sigma), _ptr(grad_params), _ptr(d_pts), None, reuse, flags, _ptr(ent["buf"]), need,
                                          _event(input_grad_event), _stream()), "lnr_density_backward")
        return d_pts
    rays, z = _f32c(rays), _f32c(z)
    n, s = z.shape
    reuse = int(bool(reuse_features))
    if reuse and ent["features_of"] != (params.data_ptr(), rays.data_ptr(), z.data_ptr(), n * s):
        raise RuntimeError("density_backward(reuse_features=True): workspace features belong to a different forward call")
    d_pts = torch.empty(n, s, 3, device=params.device, dtype=torch.float32) if want_d_pts else None
    check(load().lnr_density_backward(C.byref(spec), _ptr(params), None, 0, _ptr(rays), _ptr(z), n, s,
                                      _ptr(n_rays_dev), _ptr(d_sigma), _ptr(grad_params), _ptr(d_pts), _ptr(d_rays), reuse, flags,
                                      _ptr(ent["buf"]), need, _event(input_grad_event), _stream()), "lnr_density_backward")
    return d_pts


def density_fold_weight_grads(spec, grad_params, n_points, overwrite_grad=False):
    """Adds the weight-gradient slabs a density_backward(defer_weight_fold=True) call left in the workspace to grad_params
    (on the current stream: the training loop does it on its side stream, beside the table-gradient reduce)."""
    require_device(grad_params)
    ent, need = _workspace(spec, grad_params.device, n_points)
    check(load().lnr_density_fold_weight_grads(C.byref(spec), int(n_points), _ptr(grad_params), _ptr(ent["buf"]), need,
                                               hip.BWD_OVERWRITE_GRAD if overwrite_grad else 0, _stream()),
          "lnr_density_fold_weight_grads")


# ---------------------------------------------------------------- rays
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
    sh = (C.c_float * 3)(float(shift[0]), float(shift[1]), float(shift[2]))
    check(load().lnr_build_lidar_rays(_ptr(directions), _ptr(distances), directions.shape[1], _ptr(index), m,
                                      _ptr(transform12), float(ray_range[0]), float(ray_range[1]), float(scale), sh,
                                      _ptr(rays), _ptr(depths), _ptr(keep), _stream()), "lnr_build_lidar_rays")
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
    sh = (C.c_float * 3)(float(shift[0]), float(shift[1]), float(shift[2]))
    check(load().lnr_build_camera_rays(_ptr(directions), n_pixels, _ptr(index), n, int(width), _ptr(transform12), float(range_min),
                                       float(scale), sh, _ptr(rays), _stream()), "lnr_build_camera_rays")
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
    sh = (C.c_float * 3)(float(shift[0]), float(shift[1]), float(shift[2]))
    check(load().lnr_build_window_rays(tab.dirs, tab.dist, tab.const_dist, tab.n_points, tab.seg_start, tab.seg_pose, tab.n_seg,
                                       _ptr(index), _ptr(idx_out), int(seed) & (2 ** 64 - 1), _ptr(_f32c(transforms)),
                                       float(ray_range[0]), float(ray_range[1]), float(scale), sh, _ptr(rays), _ptr(depths),
                                       _ptr(keep), _stream()), "lnr_build_window_rays")
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
    check(load().lnr_pose_backward(_ptr(p), _ptr(_f32c(d_transforms)), _ptr(mask), p.shape[0], _ptr(out), int(accumulate),
                                   _ptr(poison), int(poison_tag), _stream()), "lnr_pose_backward")
    return out


def compact_rays(rays, depths, keep, src_index, seg_start, n_out=None, want_counts=False, front=None):
    """seg_start: python list [n_seg+1] (or the ctypes int32 array of a WindowTables).  -> (rays_out [cap,13], depths_out, src_out, out_seg_start dev int32
    [n_seg+1], n_out dev int32 [1]); only the first n_out rows are meaningful.  n_out (optional): an int32 [1] device tensor the
    live count is written into (the training loop hands in a row of its per-iteration log instead of copying into it afterwards).
    want_counts / front = (seg_order ctypes array or list, cap): the same launch also computes count_opaque's {#rays, #opaque rays} /
    writes the rank's front record (shard_front_pack) - a sixth return value, counts int32 [2] or record float32 [FRONT_HEADER + cap]."""
    require_device(rays, depths, keep, src_index)
    n_in = rays.shape[0]
    dev = rays.device
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
        check(load().lnr_compact_rays_front(_ptr(rays), _ptr(depths), _ptr(keep), _ptr(src_index), n_in, seg, n_seg,
                                            _ptr(rays_out), _ptr(depths_out), _ptr(src_out), _ptr(out_seg), _ptr(n_out),
                                            _ptr(counts), order, int(cap), _ptr(rec), _stream()), "lnr_compact_rays_front")
        return rays_out, depths_out, src_out, out_seg, n_out, (rec if front is not None else counts)
    check(load().lnr_compact_rays(_ptr(rays), _ptr(depths), _ptr(keep), _ptr(src_index), n_in, seg, n_seg,
                                  _ptr(rays_out), _ptr(depths_out), _ptr(src_out), _ptr(out_seg), _ptr(n_out), _stream()),
          "lnr_compact_rays")
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
    check(load().lnr_shard_front_pack(_ptr(rays), _ptr(out_seg_start), order, n_seg, _ptr(_f32c(depths)), rays.shape[0], _ptr(n_rays_dev),
                                      int(cap), _ptr(rec), _stream()), "lnr_shard_front_pack")
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
    check(load().lnr_lidar_rays_backward(_ptr(_f32c(d_rays)), _ptr(rays), _ptr(src_index), _ptr(seg_start_dev), n_seg, ptrs,
                                         npts, _ptr(_f32c(transforms)), float(scale), _ptr(out), _stream()),
          "lnr_lidar_rays_backward")
    return out


# ---------------------------------------------------------------- samplers
def occ_interpolate(grid, pts):
    require_device(grid, pts)
    v = grid.shape[-1]
    g = _f32c(grid).reshape(v, v, v)
    p = _f32c(pts)
    out = torch.empty(p.shape[:-1], device=p.device, dtype=torch.float32)
    check(load().lnr_occ_interpolate(_ptr(g), v, _ptr(p), out.numel(), _ptr(out), _stream()), "lnr_occ_interpolate")
    return out


def sample_rays_occ(rays, grid, n_samples, perturb, u_jitter=None, u_pdf=None, seed=0, n_rays_dev=None, debug=False):
    require_device(rays, grid, u_jitter, u_pdf)
    rays = _f32c(rays)
    v = grid.shape[-1]
    g = _f32c(grid).reshape(v, v, v)
    n = rays.shape[0]
    h = n_samples // 2
    steps = linspace_table(h, rays.device)
    z = torch.empty(n, n_samples, device=rays.device, dtype=torch.float32)
    inds = probs = cdf = None
    if debug:
        inds = torch.zeros(n, h, device=rays.device, dtype=torch.int64)
        probs = torch.zeros(n, h, device=rays.device, dtype=torch.float32)
        cdf = torch.zeros(n, h - 1, device=rays.device, dtype=torch.float32)
    check(load().lnr_sample_rays_occ(_ptr(rays), n, _ptr(n_rays_dev), _ptr(g), v, n_samples, float(perturb), _ptr(steps),
                                     _ptr(_f32c(u_jitter)), _ptr(_f32c(u_pdf)), int(seed) & (2 ** 64 - 1), _ptr(z),
                                     _ptr(inds), _ptr(probs), _ptr(cdf), _stream()), "lnr_sample_rays_occ")
    if debug:
        return z, dict(inds=inds, probs=probs, cdf=cdf)
    return z


def sample_rays_uniform(rays, n_samples, perturb, u_jitter=None, seed=0, n_rays_dev=None):
    require_device(rays, u_jitter)
    rays = _f32c(rays)
    n = rays.shape[0]
    steps = linspace_table(n_samples, rays.device)
    z = torch.zeros(n, n_samples, device=rays.device, dtype=torch.float32)
    check(load().lnr_sample_rays_uniform(_ptr(rays), n, _ptr(n_rays_dev), n_samples, float(perturb), _ptr(steps),
                                         _ptr(_f32c(u_jitter)), int(seed) & (2 ** 64 - 1), _ptr(z), _stream()),
          "lnr_sample_rays_uniform")
    return z


# ---------------------------------------------------------------- rendering
def ftb_gather(rays, z, idx, n_alive, b0, block, rays_c, z_c, next_count):
    """front-to-back inference (lnr_render_ftb_gather): alive rays' records and block depths -> the compact arrays rays_c / z_c"""
    require_device(rays, z, idx, n_alive, rays_c, z_c, next_count)
    check(load().lnr_render_ftb_gather(_ptr(rays), _ptr(z), z.shape[1], _ptr(idx), _ptr(n_alive), rays.shape[0], int(b0), int(block),
                                       _ptr(rays_c), _ptr(z_c), _ptr(next_count), _stream()), "lnr_render_ftb_gather")


def ftb_composite(sigma_c, z, rays, idx, n_alive, b0, block, noise_std, seed, transmittance, depth_acc, opacity_acc, next_idx, next_count, last, noise=None):
    """front-to-back inference (lnr_render_ftb_composite): one block's contributions of the alive rays; survivors appended to next_idx"""
    require_device(sigma_c, z, rays, idx, n_alive, transmittance, depth_acc, opacity_acc, next_idx, next_count, noise)
    check(load().lnr_render_ftb_composite(_ptr(sigma_c), _ptr(z), _ptr(rays), z.shape[1], _ptr(idx), _ptr(n_alive), rays.shape[0], int(b0), int(block),
                                          _ptr(_f32c(noise) if noise is not None else None), float(noise_std), int(seed), _ptr(transmittance), _ptr(depth_acc), _ptr(opacity_acc), _ptr(next_idx),
                                          _ptr(next_count), 1 if last else 0, _stream()), "lnr_render_ftb_composite")


def render_forward(sigma, z, rays, noise=None, noise_std=0.0, seed=0, n_rays_dev=None, want_weights=True):
    """-> (depth, weights, opacity, variance); want_weights=False leaves the [n, S] weights unwritten (returns None for them)."""
    require_device(sigma, z, rays, noise)
    sigma, z, rays = _f32c(sigma), _f32c(z), _f32c(rays)
    n, s = z.shape
    dev = z.device
    depth = torch.zeros(n, device=dev); opacity = torch.zeros(n, device=dev); variance = torch.zeros(n, device=dev)
    weights = torch.zeros(n, s, device=dev) if want_weights else None
    check(load().lnr_render_forward(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)),
                                    float(noise_std), int(seed), _ptr(depth), _ptr(weights), _ptr(opacity), _ptr(variance),
                                    _stream()), "lnr_render_forward")
    return depth, weights, opacity, variance


def render_forward_peak(sigma, z, rays, noise=None, noise_std=0.0, seed=0, n_rays_dev=None):
    """-> (depth, opacity, variance, peak_z, peak_index int32): render_forward's depth, opacity and variance bit for bit, and per ray
    the sample of maximal weight (torch.argmax's rules) with its depth - no [n, S] weights (lnr_render_forward_peak)."""
    require_device(sigma, z, rays, noise)
    sigma, z, rays = _f32c(sigma), _f32c(z), _f32c(rays)
    n, s = z.shape
    dev = z.device
    depth = torch.zeros(n, device=dev); opacity = torch.zeros(n, device=dev); variance = torch.zeros(n, device=dev)
    peak_z = torch.zeros(n, device=dev)
    peak_index = torch.zeros(n, device=dev, dtype=torch.int32)
    check(load().lnr_render_forward_peak(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)),
                                         float(noise_std), int(seed), _ptr(depth), _ptr(opacity), _ptr(variance), _ptr(peak_z),
                                         _ptr(peak_index), _stream()), "lnr_render_forward_peak")
    return depth, opacity, variance, peak_z, peak_index


def depth_colormap(values, table, multiplier=1.0, min_depth=1.0, max_depth=50.0):
    """fp32 values of any shape -> uint8 [..., 4] RGBA (lnr_depth_colormap: the reference's save_depth per element).  table: uint8
    [256,3] on the device."""
    require_device(values, table)
    values = _f32c(values)
    assert table.dtype == torch.uint8 and table.is_contiguous() and tuple(table.shape) == (256, 3)
    if not float(max_depth) > float(min_depth):
        raise ValueError(f"depth_colormap: max_depth must exceed min_depth, got {min_depth!r} and {max_depth!r}")
    rgba = torch.empty(tuple(values.shape) + (4,), device=values.device, dtype=torch.uint8)
    check(load().lnr_depth_colormap(_ptr(values), values.numel(), float(multiplier), float(min_depth), float(max_depth), _ptr(table),
                                    _ptr(rgba), _stream()), "lnr_depth_colormap")
    return rgba


class MeshLattice:
    """The mesher's lattice on a device (include/loner_hip.h: LnrMeshGrid): the three np.linspace axes (fp64, kept alive here) and
    the bound of the reference's fp32 bound check.  axes: three 1-D float64 arrays; bound: [[lo, hi]] x 3 (float64, world-cube units)."""

    def __init__(self, axes, bound, device):
        import numpy as np
        self.axes = [torch.as_tensor(np.asarray(a, dtype=np.float64)).to(device).contiguous() for a in axes]
        self.shape = tuple(int(a.numel()) for a in self.axes)            # (nx, ny, nz)
        g = hip.MeshGrid()
        for i, a in enumerate(axes):
            a = np.asarray(a, dtype=np.float64)
            g.n[i] = a.shape[0]
            g.lo[i] = float(np.float32(bound[i][0]))                     # the 0-dim fp64 bound meets fp32 points: compared in fp32
            g.hi[i] = float(np.float32(bound[i][1]))
            g.first[i] = float(a[0])
            g.inv_step[i] = float(1.0 / (a[1] - a[0])) if a.shape[0] > 1 and a[1] != a[0] else 0.0
            g.axis[i] = self.axes[i].data_ptr()
        self.grid = g

    @property
    def n_nodes(self):
        return self.shape[0] * self.shape[1] * self.shape[2]


def mesh_accumulate(sigma, z, rays, lattice: MeshLattice, volume, depth_max, var_max=None, noise=None, noise_std=0.0, seed=0,
                    n_rays_dev=None, counters=None):
    """Renders the rays (lnr_render_forward's arithmetic) and max-accumulates every sample's weight into volume [ny*nx*nz] fp32 (the
    reference's [y][x][z] order, include/loner_hip.h: lnr_render_mesh_accumulate).  counters: optional int64 [2] += {samples that
    reached the volume, atomics issued}."""
    require_device(sigma, z, rays, volume, noise, counters)
    sigma, z, rays = _f32c(sigma), _f32c(z), _f32c(rays)
    assert volume.dtype == torch.float32 and volume.is_contiguous() and volume.numel() == lattice.n_nodes
    assert counters is None or (counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == 2)
    n, s = z.shape
    check(load().lnr_render_mesh_accumulate(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)), float(noise_std),
                                            int(seed), C.byref(lattice.grid), float(depth_max), 0 if var_max is None else 1,
                                            0.0 if var_max is None else float(var_max), _ptr(volume), _ptr(counters), _stream()),
          "lnr_render_mesh_accumulate")
    return volume


def mc_case_table():
    """The marching-cubes case table as numpy int8 [256, MC_TABLE_WIDTH] (host: no device needed)."""
    import numpy as np
    out = np.empty((256, hip.MC_TABLE_WIDTH), dtype=np.int8)
    check(load().lnr_mc_case_table(out.ctypes.data_as(C.c_void_p)), "lnr_mc_case_table")
    return out


def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), valid=None):
    """Marching cubes of a device volume [nx, ny, nz] at `level` (inside: v > level) -> (verts [V,3] fp32, faces [F,3] int32) on the
    device; both empty when nothing crosses the level.  Vertex i lies at index * spacing + origin (include/loner_hip.h: lnr_mc_*).
    One device -> host read of the two totals sizes the outputs.
    valid (uint8 or bool [nx, ny, nz] on the volume's device, optional): the nodes that were observed (lnr_mc_*_masked); a cell with a
    corner that is not valid emits nothing, and vertices no surviving cell uses may remain (mesh_select(drop_unreferenced=True))."""
    require_device(volume)
    vol = _f32c(volume)
    assert vol.dim() == 3, "marching_cubes: a 3-D volume [nx, ny, nz]"
    nx, ny, nz = (int(x) for x in vol.shape)
    dev = vol.device
    if valid is not None:
        require_device(valid)
        if tuple(valid.shape) != (nx, ny, nz) or valid.dtype not in (torch.uint8, torch.bool) or valid.device != dev:
            raise ValueError(f"marching_cubes: valid must be uint8 or bool [{nx},{ny},{nz}] on {dev}, got {valid.dtype} "
                             f"{tuple(valid.shape)} on {valid.device}")
        mask = valid.to(torch.uint8).contiguous()
    lib = load()
    ws_bytes = lib.lnr_mc_workspace(nx, ny, nz)
    ws = torch.empty(max(int(ws_bytes), 1), device=dev, dtype=torch.uint8)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    if valid is None:
        check(lib.lnr_mc_count(_ptr(vol), nx, ny, nz, float(level), _ptr(ws), int(ws_bytes), _ptr(totals), _stream()), "lnr_mc_count")
    else:
        check(lib.lnr_mc_count_masked(_ptr(vol), _ptr(mask), nx, ny, nz, float(level), _ptr(ws), int(ws_bytes), _ptr(totals), _stream()),
              "lnr_mc_count_masked")
    n_verts, n_tris = (int(x) for x in totals.cpu())
    if n_verts >= 1 << 30:                          # lnr_mc_emit's limit: refused before the outputs are allocated
        raise RuntimeError(f"marching_cubes: {n_verts} vertices, the limit is 2^30 - 1")
    verts = torch.empty(n_verts, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_tris, 3, device=dev, dtype=torch.int32)
    sp = (C.c_float * 3)(*[float(x) for x in spacing])
    org = (C.c_float * 3)(*[float(x) for x in origin])
    if valid is None:
        check(lib.lnr_mc_emit(_ptr(vol), nx, ny, nz, float(level), sp, org, _ptr(ws), int(ws_bytes), n_verts, n_tris, _ptr(verts),
                              _ptr(faces), _stream()), "lnr_mc_emit")
    else:
        check(lib.lnr_mc_emit_masked(_ptr(vol), _ptr(mask), nx, ny, nz, float(level), sp, org, _ptr(ws), int(ws_bytes), n_verts, n_tris,
                                     _ptr(verts), _ptr(faces), _stream()), "lnr_mc_emit_masked")
    return verts, faces


# ---------------------------------------------------------------- point clouds
_cloud_ws = {}


def _cloud_workspace(n, device):
    """lnr_cloud_workspace(n) bytes on `device`: one buffer per device, grown on demand (calls on one stream reuse it in order)."""
    need = int(load().lnr_cloud_workspace(int(n)))
    if need == 0:
        raise RuntimeError(f"point clouds: {n} points, the limit per call is 2^31 - 4096")
    key = str(device)
    buf = _cloud_ws.get(key)
    if buf is None or buf.numel() < need:
        _cloud_ws.pop(key, None)
        buf = _cloud_ws[key] = torch.empty(need, device=device, dtype=torch.uint8)
    return buf, need


def _f64_points(t, what):
    require_device(t)
    assert t.dim() == 2 and t.shape[1] == 3, f"{what}: points [n,3]"
    return t.to(torch.float64).contiguous()


_CLOUD_STATUS = {1: "non-finite input coordinates", 2: "voxel_size is too small", 4: "the voxel key needs more than 64 bits"}


def _cloud_status(what, info):
    status = int(info[0])
    if status & 1:
        raise RuntimeError(f"{what}: {int(info[2])} points with non-finite coordinates")
    if status:
        raise RuntimeError(f"{what}: " + ", ".join(m for b, m in _CLOUD_STATUS.items() if status & b))


def lidar_scan_points(depth, variance, ray_index, directions, scale, var_max, depth_max):
    """Scan points of one rendered pose (include/loner_hip.h: lnr_lidar_scan_points) -> (points [m,3] fp64, count int32 [1]); the
    first count rows hold the kept rays' points in ray order, and the count stays on the device."""
    require_device(depth, variance, ray_index, directions)
    depth, variance, directions = _f32c(depth).reshape(-1), _f32c(variance).reshape(-1), _f32c(directions)
    ray_index = ray_index.to(torch.int64).contiguous()
    assert directions.dim() == 2 and directions.shape[0] == 3, "lidar_scan_points: directions [3, N]"
    m = depth.shape[0]
    assert variance.shape[0] == m and ray_index.shape[0] == m
    dev = depth.device
    ws, need = _cloud_workspace(m, dev)
    points = torch.empty(m, 3, device=dev, dtype=torch.float64)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    check(load().lnr_lidar_scan_points(_ptr(depth), _ptr(variance), _ptr(ray_index), m, _ptr(directions), directions.shape[1],
                                       float(scale), float(var_max), float(depth_max), _ptr(ws), need, _ptr(points), _ptr(count),
                                       _stream()), "lnr_lidar_scan_points")
    return points, count


def voxel_down_sample(points, voxel_size, count=None):
    """open3d's VoxelDownSample with a defined order (include/loner_hip.h: lnr_voxel_down_sample): points [n,3] (fp64), count
    (optional int32 [1] on the device) the live rows -> [k,3] fp64, one point per occupied voxel in ascending (i_x, i_y, i_z)
    order.  One device -> host read."""
    v = float(voxel_size)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"voxel_down_sample: voxel_size must be finite and > 0, got {voxel_size!r}")
    pts = _f64_points(points, "voxel_down_sample")
    require_device(count)
    n = pts.shape[0]
    dev = pts.device
    ws, need = _cloud_workspace(n, dev)
    out = torch.empty(n, 3, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    check(load().lnr_voxel_down_sample(_ptr(pts), n, _ptr(count), v, _ptr(ws), need, _ptr(out), _ptr(info), _stream()),
          "lnr_voxel_down_sample")
    info = info.cpu()
    _cloud_status("voxel_down_sample", info)
    return out[:int(info[1])]


def affine_f64(T, what, finite=False):
    """T (a tensor or an array of any float dtype) as a numpy fp64 4x4 whose bottom row is [0, 0, 0, 1] (and finite, when asked);
    ValueError(f"{what}, got ...") otherwise."""
    import numpy as np
    T = np.asarray(T.detach().cpu().numpy() if torch.is_tensor(T) else T, dtype=np.float64)
    if T.shape != (4, 4) or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) or (finite and not np.isfinite(T).all()):
        raise ValueError(f"{what}, got {T.tolist()}")
    return T


def _read_counters(device, call, what):
    """The int64 [4] counters of a grid query: allocated on `device`, filled by call(pointer), read once -> a host tensor."""
    counters = torch.empty(4, device=device, dtype=torch.int64)
    check(call(_ptr(counters)), what)
    return counters.cpu()


def cloud_transform(points, T, out=None):
    """out[i] = T[:3,:3] p_i + T[:3,3] in fp64 without fma (include/loner_hip.h: lnr_cloud_append_transformed).  T: a 4x4 affine
    (tensor or array, any float dtype, widened to fp64); out (optional, [n,3] fp64, may be `points` itself or a slice of a larger
    cloud) receives the result."""
    T = affine_f64(T, "transform: T must be a 4x4 affine matrix with bottom row [0, 0, 0, 1]")
    pts = _f64_points(points, "transform")
    out = torch.empty_like(pts) if out is None else out
    assert out.dtype == torch.float64 and out.is_contiguous() and out.shape == pts.shape
    t12 = (C.c_double * 12)(*[float(x) for x in T[:3].reshape(-1)])
    check(load().lnr_cloud_append_transformed(_ptr(pts), pts.shape[0], t12, _ptr(out), _stream()), "lnr_cloud_append_transformed")
    return out


class NNGrid:
    """The nearest-neighbour grid over a target cloud (include/loner_hip.h: lnr_nn_grid_build), reusable for any number of query
    batches.  cell_edge: None for the default rule.  .edge, .n_cells, .dims: what the build chose (one host read)."""

    def __init__(self, targets, cell_edge=None):
        pts = _f64_points(targets, "NNGrid")
        self.n = pts.shape[0]
        dev = pts.device
        lib = load()
        gbytes = int(lib.lnr_nn_grid_bytes(self.n))
        if gbytes == 0:
            raise RuntimeError(f"NNGrid: {self.n} targets, the limit is 2^31 - 4096")
        self.buf = torch.empty(gbytes, device=dev, dtype=torch.uint8)
        ws, need = _cloud_workspace(self.n, dev)
        info = torch.empty(8, device=dev, dtype=torch.int64)
        edge = 0.0 if cell_edge is None else float(cell_edge)
        if not math.isfinite(edge) or edge < 0:
            raise ValueError(f"NNGrid: cell_edge must be finite and > 0, got {cell_edge!r}")
        check(lib.lnr_nn_grid_build(_ptr(pts), self.n, edge, _ptr(ws), need, _ptr(self.buf), gbytes, _ptr(info), _stream()),
              "lnr_nn_grid_build")
        info = info.cpu()
        _cloud_status("NNGrid", info)
        self.n_cells = int(info[1])
        self.edge = float(info[4:5].view(torch.float64)[0])
        self.dims = tuple(int(x) for x in info[5:8])

    def distance(self, queries, want_sq=False, stats=None):
        """-> distance [m] fp64 to the nearest target (and d2 when want_sq); stats (a dict, optional) receives the counters
        {"fallback": queries that took the exact pass, "shells": shells visited}.  One device -> host read."""
        q = _f64_points(queries, "NNGrid.distance")
        m = q.shape[0]
        dev = q.device
        dist = torch.empty(m, device=dev, dtype=torch.float64)
        d2 = torch.empty(m, device=dev, dtype=torch.float64) if want_sq else None
        ws, need = _cloud_workspace(m, dev)
        c = _read_counters(dev, lambda counters: load().lnr_nn_distance(_ptr(self.buf), self.n, _ptr(q), m, _ptr(dist), _ptr(d2), _ptr(ws),
                                                                        need, counters, _stream()), "lnr_nn_distance")
        if int(c[1]):
            raise RuntimeError(f"compute_point_cloud_distance: {int(c[1])} queries with non-finite coordinates")
        if stats is not None:
            stats.update(fallback=int(c[0]), shells=int(c[2]))
        return (dist, d2) if want_sq else dist

    def normals(self, knn=30, want_covariances=False, stats=None):
        """open3d's EstimateNormals(KDTreeSearchParamKNN(knn)) over the grid's own targets (include/loner_hip.h: lnr_cloud_normals)
        -> normals [n,3] fp64 in the targets' order, and covariances [n,3,3] when asked; stats (a dict, optional) receives
        {"fallback", "shells"}.  One device -> host read."""
        knn = int(knn)
        if not 1 <= knn <= hip.KNN_MAX:
            raise ValueError(f"normals: knn must be in [1, {hip.KNN_MAX}], got {knn}")
        dev = self.buf.device
        normals = torch.empty(self.n, 3, device=dev, dtype=torch.float64)
        cov = torch.empty(self.n, 3, 3, device=dev, dtype=torch.float64) if want_covariances else None
        ws, need = _cloud_workspace(self.n, dev)
        c = _read_counters(dev, lambda counters: load().lnr_cloud_normals(_ptr(self.buf), self.n, knn, _ptr(normals), _ptr(cov), _ptr(ws),
                                                                          need, counters, _stream()), "lnr_cloud_normals")
        if int(c[1]):
            raise RuntimeError("normals: the grid is unusable (non-finite targets)")
        if stats is not None:
            stats.update(fallback=int(c[0]), shells=int(c[2]))
        return (normals, cov) if want_covariances else normals

    def knn_mean_distance(self, nb_neighbors=20, stats=None):
        """The mean distance of every target to its nb_neighbors nearest targets, itself included (include/loner_hip.h:
        lnr_cloud_knn_mean_distance) -> fp64 [n] in the targets' order; stats as normals'.  One device -> host read."""
        k = int(nb_neighbors)
        if not 1 <= k <= hip.KNN_MAX:
            raise ValueError(f"knn_mean_distance: nb_neighbors must be in [1, {hip.KNN_MAX}], got {nb_neighbors}")
        dev = self.buf.device
        avg = torch.empty(self.n, device=dev, dtype=torch.float64)
        ws, need = _tools_workspace(self.n, dev)
        c = _read_counters(dev, lambda counters: load().lnr_cloud_knn_mean_distance(_ptr(self.buf), self.n, k, _ptr(avg), _ptr(ws), need,
                                                                                    counters, _stream()), "lnr_cloud_knn_mean_distance")
        if int(c[1]):
            raise RuntimeError("knn_mean_distance: the grid is unusable (non-finite targets)")
        if stats is not None:
            stats.update(fallback=int(c[0]), shells=int(c[2]))
        return avg

    def outlier_threshold(self, mean_distance, std_ratio):
        """open3d's statistical-outlier threshold over knn_mean_distance's values (include/loner_hip.h: lnr_cloud_outlier_threshold)
        -> fp64 [4] on the device: {mean, std, threshold, valid}.  No host read."""
        avg = mean_distance
        require_device(avg)
        if avg.dtype != torch.float64 or avg.shape != (self.n,) or not avg.is_contiguous():
            raise ValueError(f"outlier_threshold: mean_distance fp64 [{self.n}], got {tuple(avg.shape)} {avg.dtype}")
        ratio = float(std_ratio)
        if not math.isfinite(ratio):
            raise ValueError(f"outlier_threshold: std_ratio must be finite, got {std_ratio!r}")
        ws, need = _tools_workspace(self.n, avg.device)
        res = torch.empty(4, device=avg.device, dtype=torch.float64)
        check(load().lnr_cloud_outlier_threshold(_ptr(self.buf), _ptr(avg), self.n, ratio, _ptr(ws), need, _ptr(res), _stream()),
              "lnr_cloud_outlier_threshold")
        return res

    def correspondences(self, queries, max_distance):
        """-> (index int32 [m]: the nearest target with d2 < max_distance^2, lower index on ties, -1 for none; d2 [m] fp64, +inf for
        none) (include/loner_hip.h: lnr_icp_correspondences)."""
        q = _f64_points(queries, "NNGrid.correspondences")
        r = float(max_distance)
        if not (math.isfinite(r) and r > 0):
            raise ValueError(f"correspondences: max_distance must be finite and > 0, got {max_distance!r}")
        m = q.shape[0]
        index = torch.empty(m, device=q.device, dtype=torch.int32)
        d2 = torch.empty(m, device=q.device, dtype=torch.float64)
        counters = torch.empty(4, device=q.device, dtype=torch.int64)
        check(load().lnr_icp_correspondences(_ptr(self.buf), self.n, _ptr(q), m, r, _ptr(index), _ptr(d2), _ptr(counters), _stream()),
              "lnr_icp_correspondences")
        if int(counters[1].item()):
            raise RuntimeError(f"correspondences: {int(counters[1].item())} queries with non-finite coordinates")
        return index, d2


_ICP_STATUS = {1: "non-finite source points", 2: "the target grid is unusable (non-finite targets)", 4: "non-finite target normals",
               8: "the update is not finite (a degenerate system)"}


def icp_point_to_plane(grid, target_normals, source, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                       max_iteration=30):
    """open3d's registration_icp with TransformationEstimationPointToPlane (include/loner_hip.h: lnr_icp_point_to_plane).  grid: an
    NNGrid over the targets; target_normals [n,3] in the targets' order; source [m,3]; init 4x4 (default identity).  -> dict with
    transformation (numpy fp64 4x4), fitness, inlier_rmse, n_correspondences, iterations, and the last solved system (JTJ 6x6, JTr,
    sum_d2, x).  Every round is enqueued at once; one device -> host read.  Raises RuntimeError on a status bit."""
    import numpy as np
    src = _f64_points(source, "icp_point_to_plane")
    nrm = _f64_points(target_normals, "icp_point_to_plane")
    if nrm.shape[0] != grid.n:
        raise ValueError(f"icp_point_to_plane: {nrm.shape[0]} normals for {grid.n} targets")
    r = float(max_distance)
    if not (math.isfinite(r) and r > 0):
        raise ValueError(f"icp_point_to_plane: max_correspondence_distance must be finite and > 0, got {max_distance!r}")
    T0 = affine_f64(np.eye(4) if init is None else init, "icp_point_to_plane: init must be a finite 4x4 affine matrix", finite=True)
    dev = src.device
    lib = load()
    need = int(lib.lnr_icp_workspace(src.shape[0]))
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    result = torch.empty(hip.ICP_RESULT, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    t16 = (C.c_double * 16)(*[float(x) for x in T0.reshape(-1)])
    check(lib.lnr_icp_point_to_plane(_ptr(grid.buf), grid.n, _ptr(nrm), _ptr(src), src.shape[0], r, t16, float(relative_fitness),
                                     float(relative_rmse), int(max_iteration), _ptr(ws), need, _ptr(result), _ptr(info), _stream()),
          "lnr_icp_point_to_plane")
    res = result.cpu().numpy()
    info = [int(x) for x in info.cpu()]
    if info[0]:
        raise RuntimeError("icp_point_to_plane: " + ", ".join(m for b, m in _ICP_STATUS.items() if info[0] & b))
    JTJ = np.zeros((6, 6))
    JTJ[np.triu_indices(6)] = res[18:39]
    JTJ = JTJ + np.triu(JTJ, 1).T
    return {"transformation": res[:16].reshape(4, 4).copy(), "fitness": float(res[16]), "inlier_rmse": float(res[17]),
            "n_correspondences": info[1], "iterations": info[2], "JTJ": JTJ, "JTr": res[39:45].copy(), "sum_d2": float(res[45]),
            "x": res[46:52].copy(), "system_correspondences": info[5]}


# ---------------------------------------------------------------- mesh sampling, trajectory transform
def _tools_workspace(n, device):
    """(buffer, bytes) for the entries that take lnr_cloud_tools_workspace(n) bytes: a buffer per call (the caching allocator's, so
    calls on different streams never share one)"""
    need = int(load().lnr_cloud_tools_workspace(int(n)))
    if need == 0:
        raise RuntimeError(f"{n} points, the limit is 2^31 - 4096")
    return torch.empty(need, device=device, dtype=torch.uint8), need


_MESH_STATUS = {1: "a triangle uses a non-finite vertex", 2: "a vertex index is out of range", 4: "the total area is not finite"}


def mesh_sample_points(vertices, triangles, n_points, seed=0, want_triangles=False, info=None):
    """open3d's sample_points_uniformly with a defined order (include/loner_hip.h: lnr_mesh_sample_points): vertices [V,3] (fp64) and
    triangles [F,3] (int32) on the device -> points [m,3] fp64 (and the owning triangle int32 [m] when asked); m = n_points, or 0 for a
    mesh without area.  info (a dict, optional) receives {"area", "bad_triangles"}.  Raises RuntimeError on a status bit.  One
    device -> host read."""
    require_device(vertices, triangles)
    v = _f64_points(vertices, "mesh_sample_points")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int32:
        raise ValueError(f"mesh_sample_points: triangles int32 [F,3], got {tuple(triangles.shape)} {triangles.dtype}")
    tri = triangles.contiguous()
    n, seed = int(n_points), int(seed)
    if n < 0 or not 0 <= seed < 2 ** 64:
        raise ValueError(f"mesh_sample_points: n_points >= 0 and a 64-bit seed, got {n_points!r} and {seed!r}")
    dev = v.device
    lib = load()
    need = int(lib.lnr_mesh_sample_workspace(tri.shape[0]))
    if need == 0:
        raise RuntimeError(f"mesh_sample_points: {tri.shape[0]} triangles, the limit is 2^31 - 4096")
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    points = torch.empty(n, 3, device=dev, dtype=torch.float64)
    owner = torch.empty(n, device=dev, dtype=torch.int32) if want_triangles else None
    info_dev = torch.empty(8, device=dev, dtype=torch.int64)
    check(lib.lnr_mesh_sample_points(_ptr(v), v.shape[0], _ptr(tri), tri.shape[0], n, seed, _ptr(ws), need, _ptr(points), _ptr(owner),
                                     _ptr(info_dev), _stream()), "lnr_mesh_sample_points")
    host = info_dev.cpu()
    status = int(host[0])
    if status:
        raise RuntimeError(f"mesh_sample_points: {int(host[2])} bad triangles: " + ", ".join(m for b, m in _MESH_STATUS.items() if status & b))
    if info is not None:
        info.update(area=float(host[3:4].view(torch.float64)[0]), bad_triangles=int(host[2]))
    m = int(host[1])
    return (points[:m], owner[:m]) if want_triangles else points[:m]


# ---------------------------------------------------------------- mesh tools
_MESH_TOOLS_STATUS = {1: "a vertex index is out of range", 2: "a cluster id is out of range"}


def _mesh_triangles(triangles, what):
    require_device(triangles)
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int32:
        raise ValueError(f"{what}: triangles int32 [F,3], got {tuple(triangles.shape)} {triangles.dtype}")
    return triangles.contiguous()


def _mesh_tools_workspace(what, n_vertices, n_triangles, device):
    need = int(load().lnr_mesh_tools_workspace(int(n_vertices), int(n_triangles)))
    if need == 0:
        raise RuntimeError(f"{what}: {n_vertices} vertices and {n_triangles} triangles, the limits are 2^31 - 1 vertices and "
                           "3 * triangles <= 2^31 - 4096")
    return torch.empty(need, device=device, dtype=torch.uint8), need


def _mesh_tools_info(what, info_dev, messages=_MESH_TOOLS_STATUS):
    """the one device -> host read of a mesh-tools call: (a, b) of its info words; RuntimeError on a status bit"""
    host = info_dev.cpu()
    status = int(host[0])
    if status:
        raise RuntimeError(f"{what}: " + ", ".join(m for b, m in messages.items() if status & b))
    return int(host[1]), int(host[2])


def mesh_connected_triangles(triangles, n_vertices):
    """open3d's cluster_connected_triangles without the areas (include/loner_hip.h: lnr_mesh_connected_triangles): triangles [F,3]
    int32 on the device, indices in [0, n_vertices) -> (triangle_clusters int32 [F], cluster_n_triangles int32 [C]) on the device,
    clusters numbered by their smallest triangle.  Raises RuntimeError on an index out of range.  One device -> host read (C)."""
    tri = _mesh_triangles(triangles, "mesh_connected_triangles")
    f, dev = tri.shape[0], tri.device
    ws, need = _mesh_tools_workspace("mesh_connected_triangles", 0, f, dev)
    if not 0 <= int(n_vertices) < 2 ** 31:
        raise RuntimeError(f"mesh_connected_triangles: {n_vertices} vertices, the limit is 2^31 - 1")
    clusters = torch.empty(f, device=dev, dtype=torch.int32)
    sizes = torch.empty(f, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_connected_triangles(_ptr(tri), f, int(n_vertices), _ptr(ws), need, _ptr(clusters), _ptr(sizes), _ptr(info),
                                              _stream()), "lnr_mesh_connected_triangles")
    c, _ = _mesh_tools_info("mesh_connected_triangles", info)
    return clusters, sizes[:c]


def mesh_cluster_area(vertices, triangles, triangle_clusters, n_clusters):
    """The summed triangle area of every cluster in a fixed order (include/loner_hip.h: lnr_mesh_cluster_area) -> fp64 [n_clusters]
    on the device.  Raises RuntimeError on a vertex index or a cluster id out of range.  One device -> host read (the status)."""
    v = _f64_points(vertices, "mesh_cluster_area")
    tri = _mesh_triangles(triangles, "mesh_cluster_area")
    require_device(triangle_clusters)
    f, c, dev = tri.shape[0], int(n_clusters), tri.device
    if triangle_clusters.dtype != torch.int32 or tuple(triangle_clusters.shape) != (f,) or not 0 <= c <= f:
        raise ValueError(f"mesh_cluster_area: triangle_clusters int32 [{f}] and 0 <= n_clusters <= {f}, got "
                         f"{tuple(triangle_clusters.shape)} {triangle_clusters.dtype} and {n_clusters!r}")
    ws, need = _mesh_tools_workspace("mesh_cluster_area", 0, f, dev)
    area = torch.empty(c, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_cluster_area(_ptr(v), v.shape[0], _ptr(tri), f, _ptr(triangle_clusters.contiguous()), c, _ptr(ws), need,
                                       _ptr(area), _ptr(info), _stream()), "lnr_mesh_cluster_area")
    _mesh_tools_info("mesh_cluster_area", info)
    return area


def _keep_mask(mask, n, what):
    if mask is None:
        return None
    require_device(mask)
    if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (n,):
        raise ValueError(f"mesh_select: {what} bool or uint8 [{n}], got {tuple(mask.shape)} {mask.dtype}")
    return mask.to(torch.uint8).contiguous()


def mesh_select(triangles, n_vertices, triangle_keep=None, vertex_keep=None, drop_unreferenced=False):
    """The compaction behind the mesh filters (include/loner_hip.h: lnr_mesh_select): triangles [F,3] int32, optional keep masks
    (bool or uint8) per triangle and per vertex -> (the surviving triangles [F',3] int32 re-indexed, vertex_map int32 [V] with the
    new index or -1, the number of surviving vertices).  Raises RuntimeError on an index out of range.  One device -> host read."""
    tri = _mesh_triangles(triangles, "mesh_select")
    f, v, dev = tri.shape[0], int(n_vertices), tri.device
    tk, vk = _keep_mask(triangle_keep, f, "triangle_keep"), _keep_mask(vertex_keep, v, "vertex_keep")
    ws, need = _mesh_tools_workspace("mesh_select", v, f, dev)
    out = torch.empty(f, 3, device=dev, dtype=torch.int32)
    vmap = torch.empty(v, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_select(_ptr(tri), f, v, _ptr(tk), _ptr(vk), 1 if drop_unreferenced else 0, _ptr(ws), need, _ptr(out),
                                 _ptr(vmap), _ptr(info), _stream()), "lnr_mesh_select")
    n_v, n_f = _mesh_tools_info("mesh_select", info)
    return out[:n_f], vmap, n_v


def mesh_vertex_normals(vertices, triangles):
    """TriangleMesh.compute_vertex_normals on the device, bit for bit (include/loner_hip.h: lnr_mesh_vertex_normals) -> fp64 [V,3].
    Raises RuntimeError on an index out of range.  One device -> host read (the status)."""
    v = _f64_points(vertices, "mesh_vertex_normals")
    tri = _mesh_triangles(triangles, "mesh_vertex_normals")
    f, dev = tri.shape[0], tri.device
    ws, need = _mesh_tools_workspace("mesh_vertex_normals", 0, f, dev)
    normals = torch.empty(v.shape[0], 3, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_vertex_normals(_ptr(v), v.shape[0], _ptr(tri), f, _ptr(ws), need, _ptr(normals), _ptr(info), _stream()),
          "lnr_mesh_vertex_normals")
    _mesh_tools_info("mesh_vertex_normals", info)
    return normals


_MESH_FILTERS_STATUS = {1: "an index is out of range"}


def _mesh_filters_workspace(what, n_vertices, n_triangles, device):
    need = int(load().lnr_mesh_filters_workspace(int(n_vertices), int(n_triangles)))
    if need == 0:
        raise RuntimeError(f"{what}: {n_vertices} vertices and {n_triangles} triangles, the limits are 2^31 - 4096 vertices and "
                           "6 * triangles <= 2^31 - 4096")
    return torch.empty(need, device=device, dtype=torch.uint8), need


def _vertex_count(n_vertices, what):
    v = int(n_vertices)
    if v != n_vertices or not 0 <= v < 2 ** 31:
        raise ValueError(f"{what}: n_vertices must be an integer in [0, 2^31 - 1], got {n_vertices!r}")
    return v


def mesh_vertex_clusters(vertices, voxel_size):
    """The vertex half of open3d's simplify_vertex_clustering with averaging (include/loner_hip.h: lnr_mesh_vertex_clusters):
    vertices [V,3] (fp64) -> (vertex_cluster int32 [V], cluster_vertices fp64 [m,3]) on the device, clusters numbered by first
    occurrence.  Raises ValueError for a voxel_size that is not finite and > 0, RuntimeError on a non-finite vertex, a voxel_size
    that is too small or a key wider than 64 bits.  One device -> host read (the status and m)."""
    s = float(voxel_size)
    if not (math.isfinite(s) and s > 0):
        raise ValueError(f"mesh_vertex_clusters: voxel_size must be finite and > 0, got {voxel_size!r}")
    v = _f64_points(vertices, "mesh_vertex_clusters")
    n, dev = v.shape[0], v.device
    ws, need = _mesh_filters_workspace("mesh_vertex_clusters", n, 0, dev)
    cluster = torch.empty(n, device=dev, dtype=torch.int32)
    means = torch.empty(n, 3, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_vertex_clusters(_ptr(v), n, s, _ptr(ws), need, _ptr(cluster), _ptr(means), _ptr(info), _stream()),
          "lnr_mesh_vertex_clusters")
    host = info.cpu()
    if int(host[0]) & 1:
        raise RuntimeError(f"mesh_vertex_clusters: {int(host[2])} vertices with non-finite coordinates")
    _cloud_status("mesh_vertex_clusters", host)
    return cluster, means[:int(host[1])]


def mesh_unique_triangles(triangles, n_vertices, vertex_map=None, n_mapped=None, drop_degenerate=False):
    """open3d's remove_duplicated_triangles as a mask (include/loner_hip.h: lnr_mesh_unique_triangles): triangles [F,3] int32,
    optional vertex_map int32 [n_vertices] with values in [0, n_mapped) -> (canonical int32 [F,3], the mapped corners rotated by
    open3d's rule; triangle_keep uint8 [F], 1 for the first triangle of each canonical triple, with drop_degenerate only where its
    three indices differ; the number kept; the number of degenerate triangles).  Raises RuntimeError on an index or a mapped value
    out of range.  One device -> host read."""
    tri = _mesh_triangles(triangles, "mesh_unique_triangles")
    f, dev = tri.shape[0], tri.device
    v = _vertex_count(n_vertices, "mesh_unique_triangles")
    if vertex_map is None:
        if n_mapped is not None and int(n_mapped) != v:
            raise ValueError(f"mesh_unique_triangles: n_mapped is n_vertices without a vertex_map, got {n_mapped!r}")
        m = v
    else:
        require_device(vertex_map)
        if vertex_map.dtype != torch.int32 or tuple(vertex_map.shape) != (v,) or n_mapped is None or not 0 <= int(n_mapped) < 2 ** 31:
            raise ValueError(f"mesh_unique_triangles: vertex_map int32 [{v}] and n_mapped in [0, 2^31 - 1], got "
                             f"{tuple(vertex_map.shape)} {vertex_map.dtype} and {n_mapped!r}")
        vertex_map, m = vertex_map.contiguous(), int(n_mapped)
    ws, need = _mesh_filters_workspace("mesh_unique_triangles", 0, f, dev)
    canonical = torch.empty(f, 3, device=dev, dtype=torch.int32)
    keep = torch.empty(f, device=dev, dtype=torch.uint8)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_unique_triangles(_ptr(tri), f, v, _ptr(vertex_map), m, 1 if drop_degenerate else 0, _ptr(ws), need,
                                           _ptr(canonical), _ptr(keep), _ptr(info), _stream()), "lnr_mesh_unique_triangles")
    n_kept, n_degenerate = _mesh_tools_info("mesh_unique_triangles", info, _MESH_FILTERS_STATUS)
    return canonical, keep, n_kept, n_degenerate


def mesh_vertex_adjacency(triangles, n_vertices):
    """Every vertex's distinct neighbours as a CSR (include/loner_hip.h: lnr_mesh_vertex_adjacency): triangles [F,3] int32 ->
    (row_start int32 [V+1], neighbours int32 [row_start[V]]) on the device, each row ascending, a vertex never its own neighbour.
    Raises RuntimeError on an index out of range.  One device -> host read (the status and the number of neighbours)."""
    tri = _mesh_triangles(triangles, "mesh_vertex_adjacency")
    f, dev = tri.shape[0], tri.device
    v = _vertex_count(n_vertices, "mesh_vertex_adjacency")
    ws, need = _mesh_filters_workspace("mesh_vertex_adjacency", 0, f, dev)
    row_start = torch.empty(v + 1, device=dev, dtype=torch.int32)
    neighbours = torch.empty(6 * f, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_vertex_adjacency(_ptr(tri), f, v, _ptr(ws), need, _ptr(row_start), _ptr(neighbours), _ptr(info), _stream()),
          "lnr_mesh_vertex_adjacency")
    n, _ = _mesh_tools_info("mesh_vertex_adjacency", info, _MESH_FILTERS_STATUS)
    return row_start, neighbours[:n]


MESH_SMOOTH_KINDS = {"simple": 0, "laplacian": 1}


def mesh_smooth(vertices, row_start, neighbours, n_steps, kind="laplacian", lambda_filter=0.5, mu=None):
    """n_steps smoothing steps on the device (include/loner_hip.h: lnr_mesh_smooth): vertices [V,3] (fp64), the adjacency of
    mesh_vertex_adjacency, kind "simple" or "laplacian"; step s uses lambda_filter when s is even and mu (default: lambda_filter)
    when s is odd, so Taubin's k iterations are 2 k Laplacian steps with mu < 0 -> a new fp64 [V,3] tensor; the input is not
    changed.  Raises RuntimeError on an adjacency entry out of range.  One device -> host read (the status)."""
    if kind not in MESH_SMOOTH_KINDS:
        raise ValueError(f"mesh_smooth: kind must be one of {sorted(MESH_SMOOTH_KINDS)}, got {kind!r}")
    steps = int(n_steps)
    if steps != n_steps or not 0 <= steps < 2 ** 31:
        raise ValueError(f"mesh_smooth: n_steps must be an integer >= 0, got {n_steps!r}")
    lam = float(lambda_filter)
    m = lam if mu is None else float(mu)
    if not (math.isfinite(lam) and math.isfinite(m)):
        raise ValueError(f"mesh_smooth: the factors must be finite, got {lambda_filter!r} and {mu!r}")
    v = _f64_points(vertices, "mesh_smooth").clone()
    require_device(row_start, neighbours)
    n, dev = v.shape[0], v.device
    if row_start.dtype != torch.int32 or tuple(row_start.shape) != (n + 1,) or neighbours.dtype != torch.int32 or neighbours.dim() != 1:
        raise ValueError(f"mesh_smooth: row_start int32 [{n + 1}] and neighbours int32 [n], got {tuple(row_start.shape)} "
                         f"{row_start.dtype} and {tuple(neighbours.shape)} {neighbours.dtype}")
    row_start, neighbours = row_start.contiguous(), neighbours.contiguous()
    scratch = torch.empty_like(v)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_smooth(_ptr(v), _ptr(scratch), n, _ptr(row_start), _ptr(neighbours), neighbours.shape[0],
                                 MESH_SMOOTH_KINDS[kind], steps, lam, m, _ptr(info), _stream()), "lnr_mesh_smooth")
    _mesh_tools_info("mesh_smooth", info, _MESH_FILTERS_STATUS)
    return v


class Trajectory:
    """A ground-truth trajectory on the device, in the form lnr_cloud_trajectory_transform takes: times [K] (strictly increasing),
    positions [K,3], rotations [K,3,3] and the rotation vectors log(R_k^T R_k+1) [K-1,3], all fp64 host arrays here."""

    def __init__(self, times, positions, rotations, rotvecs, device):
        import numpy as np
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        K = t.shape[0]
        if K < 2:
            raise ValueError(f"Trajectory: at least 2 poses are needed, got {K}")
        P = np.ascontiguousarray(positions, dtype=np.float64)
        R = np.ascontiguousarray(rotations, dtype=np.float64)
        W = np.ascontiguousarray(rotvecs, dtype=np.float64)
        if P.shape != (K, 3) or R.shape != (K, 3, 3) or W.shape != (K - 1, 3):
            raise ValueError(f"Trajectory: positions [{K},3], rotations [{K},3,3] and rotvecs [{K - 1},3], got {P.shape}, {R.shape}, {W.shape}")
        if not (np.isfinite(t).all() and np.isfinite(P).all() and np.isfinite(R).all() and np.isfinite(W).all()):
            raise ValueError("Trajectory: a pose or a pose time is not finite")
        if not (np.diff(t) > 0).all():
            raise ValueError("Trajectory: the pose times must be strictly increasing")
        self.n_poses = K
        self.t0, self.t1 = float(t[0]), float(t[-1])
        self.times, self.positions, self.rotations, self.rotvecs = (torch.from_numpy(a).to(device) for a in (t, P, R, W))


def trajectory_transform(points, timestamps, trajectory, min_range):
    """Every point moved by the trajectory's pose at its own time (include/loner_hip.h: lnr_cloud_trajectory_transform): points [n,3]
    (sensor frame), timestamps [n] (absolute, fp64), trajectory a Trajectory on the same device -> (out [n,3] fp64 whose first `kept`
    rows hold the kept points in input order, info int64 [8] on the device: {status, kept, below range, outside, non-finite})."""
    pts = _f64_points(points, "trajectory_transform")
    require_device(timestamps)
    n = pts.shape[0]
    if timestamps.shape != (n,):
        raise ValueError(f"trajectory_transform: timestamps [{n}], got {tuple(timestamps.shape)}")
    stamps = timestamps.to(torch.float64).contiguous()
    r = float(min_range)
    if math.isnan(r):
        raise ValueError("trajectory_transform: min_range is NaN")
    dev = pts.device
    ws, need = _tools_workspace(n, dev)
    out = torch.empty(n, 3, device=dev, dtype=torch.float64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    tr = trajectory
    check(load().lnr_cloud_trajectory_transform(_ptr(pts), _ptr(stamps), n, _ptr(tr.times), _ptr(tr.positions), _ptr(tr.rotations),
                                                _ptr(tr.rotvecs), tr.n_poses, r, _ptr(ws), need, _ptr(out), _ptr(info), _stream()),
          "lnr_cloud_trajectory_transform")
    return out, info


# ---------------------------------------------------------------- ray casting
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
        need, nbytes = int(lib.lnr_bvh_workspace(f)), int(lib.lnr_bvh_bytes(f))
        if need == 0 or nbytes == 0:
            raise RuntimeError(f"BVH: {f} triangles, the limit is 2^31 - 4096")
        self.n_triangles = f
        self.buf = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        info = torch.empty(hip.RAYCAST_INFO, device=dev, dtype=torch.int64)
        check(lib.lnr_bvh_build(_ptr(v), v.shape[0], _ptr(tri), f, _ptr(ws), need, _ptr(self.buf), nbytes, _ptr(info), _stream()),
              "lnr_bvh_build")
        host = info.cpu()
        status = int(host[0])
        if status:
            raise RuntimeError(f"BVH: {int(host[3])} triangles with an index out of range: " +
                               ", ".join(m for b, m in _BVH_STATUS.items() if status & b))
        self.n_in_tree, self.n_nonfinite, self.depth, self.n_nodes = int(host[1]), int(host[2]), int(host[4]), int(host[5])

    @property
    def device(self):
        return self.buf.device


def cast_rays(bvh, rays, t_min=0.0, t_max=math.inf, want_uvs=True, stats=None):
    """open3d's RaycastingScene.cast_rays with a window (include/loner_hip.h: lnr_cast_rays): rays [n,6] (ox oy oz dx dy dz) on the
    BVH's device -> (t_hit fp64 [n], +inf on a miss; primitive_ids int32 [n], -1 on a miss; primitive_uvs fp64 [n,2] or None).
    stats (a dict, optional) receives {"hits", "invalid_rays", "node_visits", "capped_rays", "excluded_triangles", "depth"} at the
    price of one device -> host read, which then also raises RuntimeError on a status bit; without it nothing is read back."""
    if not isinstance(bvh, BVH):
        raise ValueError(f"cast_rays: bvh must be an ops.BVH, got {type(bvh).__name__}")
    require_device(rays)
    if rays.dim() != 2 or rays.shape[1] != 6:
        raise ValueError(f"cast_rays: rays [n,6], got {tuple(rays.shape)}")
    lo, hi = float(t_min), float(t_max)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f"cast_rays: t_min and t_max must be numbers, got {t_min!r} and {t_max!r}")
    if rays.device != bvh.device:
        raise ValueError(f"cast_rays: rays on {rays.device}, the BVH on {bvh.device}")
    r = rays.to(torch.float64).contiguous()
    n, dev = r.shape[0], r.device
    t_hit = torch.empty(n, device=dev, dtype=torch.float64)
    ids = torch.empty(n, device=dev, dtype=torch.int32)
    uvs = torch.empty(n, 2, device=dev, dtype=torch.float64) if want_uvs else None
    info = torch.empty(hip.RAYCAST_INFO, device=dev, dtype=torch.int64)
    check(load().lnr_cast_rays(_ptr(bvh.buf), bvh.n_triangles, _ptr(r), n, lo, hi, _ptr(t_hit), _ptr(ids), _ptr(uvs), _ptr(info),
                               _stream()), "lnr_cast_rays")
    if stats is not None:
        host = info.cpu()
        status = int(host[0])
        if status:
            raise RuntimeError("cast_rays: " + ", ".join(m for b, m in _CAST_STATUS.items() if status & b))
        stats.update(hits=int(host[1]), invalid_rays=int(host[2]), node_visits=int(host[3]), capped_rays=int(host[4]),
                     excluded_triangles=int(host[5]), depth=int(host[6]))
    return t_hit, ids, uvs


def _walk_stats(what, info, stats, first, second):
    """the one host read of a BVH walk: raise on a status bit, else fill stats under the call's own names for words 1 and 2"""
    host = info.cpu()
    status = int(host[0])
    if status:
        raise RuntimeError(f"{what}: " + ", ".join(m for b, m in _CAST_STATUS.items() if status & b))
    stats.update({first: int(host[1]), second: int(host[2])}, node_visits=int(host[3]), capped=int(host[4]),
                 excluded_triangles=int(host[5]), depth=int(host[6]))


def closest_points(bvh, points, max_distance=math.inf, want_points=True, want_uvs=True, stats=None):
    """open3d's RaycastingScene.compute_closest_points with a reach (include/loner_hip.h: lnr_closest_points): points [n,3] (a float
    dtype) on the BVH's device -> (dist_sq fp64 [n], +inf with no triangle within max_distance; primitive_ids int32 [n], -1 then;
    closest fp64 [n,3] or None; primitive_uvs fp64 [n,2] or None).  stats (a dict, optional) receives {"answered", "invalid_points",
    "node_visits", "capped", "excluded_triangles", "depth"} at the price of one device -> host read, which then also raises
    RuntimeError on a status bit; without it nothing is read back."""
    if not isinstance(bvh, BVH):
        raise ValueError(f"closest_points: bvh must be an ops.BVH, got {type(bvh).__name__}")
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or not points.dtype.is_floating_point:
        raise ValueError(f"closest_points: points [n,3] of a float dtype, got {tuple(getattr(points, 'shape', ()))} "
                         f"{getattr(points, 'dtype', type(points).__name__)}")
    reach = float(max_distance)
    if math.isnan(reach) or reach < 0:
        raise ValueError(f"closest_points: max_distance must be a number >= 0, got {max_distance!r}")
    if points.device != bvh.device:
        raise ValueError(f"closest_points: points on {points.device}, the BVH on {bvh.device}")
    require_device(points)
    p = points.to(torch.float64).contiguous()
    n, dev = p.shape[0], p.device
    dist_sq = torch.empty(n, device=dev, dtype=torch.float64)
    ids = torch.empty(n, device=dev, dtype=torch.int32)
    closest = torch.empty(n, 3, device=dev, dtype=torch.float64) if want_points else None
    uvs = torch.empty(n, 2, device=dev, dtype=torch.float64) if want_uvs else None
    info = torch.empty(hip.RAYCAST_INFO, device=dev, dtype=torch.int64)
    check(load().lnr_closest_points(_ptr(bvh.buf), bvh.n_triangles, _ptr(p), n, reach * reach, _ptr(dist_sq), _ptr(ids), _ptr(closest),
                                    _ptr(uvs), _ptr(info), _stream()), "lnr_closest_points")
    if stats is not None:
        _walk_stats("closest_points", info, stats, "answered", "invalid_points")
    return dist_sq, ids, closest, uvs


def count_intersections(bvh, rays, t_min=0.0, t_max=math.inf, stats=None):
    """open3d's RaycastingScene.count_intersections with a window (include/loner_hip.h: lnr_count_intersections): rays [n,6] (a float
    dtype) on the BVH's device -> counts int32 [n], the triangles each ray crosses with t_min <= t <= t_max.  stats (a dict,
    optional) receives {"rays_crossing", "invalid_rays", "node_visits", "capped", "excluded_triangles", "depth"} at the price of one
    device -> host read, which then also raises RuntimeError on a status bit."""
    if not isinstance(bvh, BVH):
        raise ValueError(f"count_intersections: bvh must be an ops.BVH, got {type(bvh).__name__}")
    if not torch.is_tensor(rays) or rays.dim() != 2 or rays.shape[1] != 6 or not rays.dtype.is_floating_point:
        raise ValueError(f"count_intersections: rays [n,6] of a float dtype, got {tuple(getattr(rays, 'shape', ()))} "
                         f"{getattr(rays, 'dtype', type(rays).__name__)}")
    lo, hi = float(t_min), float(t_max)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f"count_intersections: t_min and t_max must be numbers, got {t_min!r} and {t_max!r}")
    if rays.device != bvh.device:
        raise ValueError(f"count_intersections: rays on {rays.device}, the BVH on {bvh.device}")
    require_device(rays)
    r = rays.to(torch.float64).contiguous()
    n, dev = r.shape[0], r.device
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    info = torch.empty(hip.RAYCAST_INFO, device=dev, dtype=torch.int64)
    check(load().lnr_count_intersections(_ptr(bvh.buf), bvh.n_triangles, _ptr(r), n, lo, hi, _ptr(counts), _ptr(info), _stream()),
          "lnr_count_intersections")
    if stats is not None:
        _walk_stats("count_intersections", info, stats, "rays_crossing", "invalid_rays")
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
    check(load().lnr_trajectory_rays(_ptr(d), _ptr(stamps), n, _ptr(tr.times), _ptr(tr.positions), _ptr(tr.rotations), _ptr(tr.rotvecs),
                                     tr.n_poses, _ptr(rays), _ptr(info), _stream()), "lnr_trajectory_rays")
    return rays, info


# ---------------------------------------------------------------- TSDF fusion
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
    if rays.dim() != 2 or rays.shape[1] != 6 or not rays.dtype.is_floating_point:
        raise ValueError(f"tsdf_integrate: rays [n,6] of a float dtype, got {tuple(rays.shape)} {rays.dtype}")
    n = rays.shape[0]
    if tuple(ranges.shape) != (n,) or not ranges.dtype.is_floating_point:
        raise ValueError(f"tsdf_integrate: ranges [{n}] of a float dtype, got {tuple(ranges.shape)} {ranges.dtype}")
    if rays.device != sum_.device or ranges.device != sum_.device:
        raise ValueError(f"tsdf_integrate: rays on {rays.device}, ranges on {ranges.device}, the volume on {sum_.device}")
    v, tr = float(voxel_size), float(trunc)
    fr = tr if front is None else float(front)
    org = [float(x) for x in origin]
    if len(org) != 3 or not all(math.isfinite(x) for x in org):
        raise ValueError(f"tsdf_integrate: origin must be three finite numbers, got {origin!r}")
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"tsdf_integrate: voxel_size must be finite and > 0, got {voxel_size!r}")
    if not (math.isfinite(tr) and tr > 0):
        raise ValueError(f"tsdf_integrate: trunc must be finite and > 0, got {trunc!r}")
    if not fr >= tr:
        raise ValueError(f"tsdf_integrate: front must be at least trunc ({tr}), got {front!r}")
    r = rays.to(torch.float64).contiguous()
    rng = ranges.to(torch.float64).contiguous()
    info = torch.empty(8, device=sum_.device, dtype=torch.int64)
    check(load().lnr_tsdf_integrate(_ptr(r), _ptr(rng), n, nx, ny, nz, (C.c_double * 3)(*org), v, tr, fr, _ptr(sum_), _ptr(count),
                                    _ptr(info), _stream()), "lnr_tsdf_integrate")
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


# ---------------------------------------------------------------- scan ingestion
_scan_ws = {}


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
    need = int(lib.lnr_scan_from_points_workspace(n))
    if need == 0:
        raise RuntimeError(f"scan_from_points: {n} points, the limit per call is 2^31 - 4096")
    ws = _scan_ws.get(str(dev))
    if ws is None or ws.numel() < need:
        _scan_ws.pop(str(dev), None)
        ws = _scan_ws[str(dev)] = torch.empty(need, device=dev, dtype=torch.uint8)
    dirs = torch.empty(3 * n, device=dev, dtype=torch.float32)
    dist = torch.empty(n, device=dev, dtype=torch.float32)
    times = torch.empty(n, device=dev, dtype=torch.float32)
    order = torch.empty(n, device=dev, dtype=torch.int64)
    info = torch.empty(8, device=dev, dtype=torch.int64)
    flat = (C.c_float * max(2 * len(segs), 1))(*[v for s in segs for v in s])
    times_in = None if mode != hip.SCAN_TIME_GIVEN else point_times.contiguous()
    check(lib.lnr_scan_from_points(_ptr(xyz.contiguous()), _ptr(times_in), n, mode, stamp, int(fov_segments is not None), flat, len(segs),
                                   min_range, _ptr(ws), need, _ptr(dirs), _ptr(dist), _ptr(times), _ptr(order), _ptr(info), _stream()),
          "lnr_scan_from_points")
    info = [int(v) for v in info.cpu()]
    m = info[0]
    return dirs[:3 * m].view(3, m), dist[:m], times[:m], order[:m], info


# ---------------------------------------------------------------- tracking
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
    check(load().lnr_frame_cloud(_ptr(_f32c(directions)), _ptr(_f32c(distances)), n, start, stop, step, _ptr(points), _stream()),
          "lnr_frame_cloud")
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
    check(load().lnr_motion_compensate(_ptr(directions), _ptr(distances), _ptr(timestamps.contiguous()),
                                       int(timestamps.dtype == torch.float64), n, float(t0), float(denom), c, _stream()),
          "lnr_motion_compensate")


_sky_ws = {}


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
    lib = load()
    need = int(lib.lnr_sky_rays_workspace())
    held = _sky_ws.get(str(dev))                # the workspace and the full-size output are kept per device; the result is copied out
    if held is None:
        held = _sky_ws[str(dev)] = (torch.empty(need, device=dev, dtype=torch.uint8),
                                    torch.empty(3, hip.SKY_MAX_RAYS, device=dev, dtype=torch.float32))
    ws, sky = held
    info = torch.empty(8, device=dev, dtype=torch.int32)
    check(lib.lnr_sky_rays(_ptr(_f32c(directions)), directions.shape[1], _ptr(rot), _ptr(ws), need, _ptr(sky), hip.SKY_MAX_RAYS,
                           _ptr(info), _stream()), "lnr_sky_rays")
    info = [int(x) for x in info.cpu()]
    if info[0]:
        raise RuntimeError(f"sky_rays: {info[6]} ray directions are not finite")
    return sky[:, :info[1]].contiguous()


def render_backward(sigma, z, rays, g_depth, g_weights, g_opacity, g_variance, noise=None, noise_std=0.0, seed=0,
                    n_rays_dev=None):
    require_device(sigma, z, rays)
    sigma, z, rays = _f32c(sigma), _f32c(z), _f32c(rays)
    n, s = z.shape
    d_sigma = torch.zeros(n, s, device=z.device)
    d_rays = torch.zeros(n, hip.RAY_STRIDE, device=z.device)
    check(load().lnr_render_backward(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)),
                                     float(noise_std), int(seed), _ptr(_f32c(g_depth)), _ptr(_f32c(g_weights)),
                                     _ptr(_f32c(g_opacity)), _ptr(_f32c(g_variance)), _ptr(d_sigma), _ptr(d_rays), _stream()),
          "lnr_render_backward")
    return d_sigma, d_rays


def points_grad_to_rays(d_pts, z, d_rays, n_rays_dev=None):
    require_device(d_pts, z, d_rays)
    n, s = z.shape
    check(load().lnr_points_grad_to_rays(_ptr(_f32c(d_pts)), _ptr(_f32c(z)), n, _ptr(n_rays_dev), s, _ptr(d_rays), _stream()),
          "lnr_points_grad_to_rays")
    return d_rays


# ---------------------------------------------------------------- loss pieces
def weights_gt(s, g, eps, normalise=True):
    require_device(s, g)
    s = _f32c(s)
    n, k = s.shape
    g = _f32c(g).reshape(-1)
    out = torch.empty_like(s)
    if isinstance(eps, torch.Tensor):
        require_device(eps)
        e = _f32c(eps).reshape(-1)
        check(load().lnr_weights_gt(_ptr(s), _ptr(g), _ptr(e), 0.0, int(normalise), n, k, _ptr(out), _stream()), "lnr_weights_gt")
    else:
        check(load().lnr_weights_gt(_ptr(s), _ptr(g), None, float(eps), int(normalise), n, k, _ptr(out), _stream()), "lnr_weights_gt")
    return out


def logits_grad(s, g, margin=2.0, l_free=0.25, l_occ=2.5):
    require_device(s, g)
    s = _f32c(s)
    n, k = s.shape
    out = torch.empty_like(s)
    check(load().lnr_logits_grad(_ptr(s), _ptr(_f32c(g).reshape(-1)), n, k, float(margin), float(l_free), float(l_occ),
                                 _ptr(out), _stream()), "lnr_logits_grad")
    return out


def count_opaque(rays, depth_gt, n_rays_dev=None, far0=None):
    """-> int32 [2] = {#rays, #opaque rays}.  far0 (device float [1], optional): the `far` every depth is compared with
    (the reference's far[0] quirk) when `rays` is only a shard of the batch."""
    require_device(rays, depth_gt, far0)
    counts = torch.empty(2, device=rays.device, dtype=torch.int32)       # overwritten, also for an empty batch
    check(load().lnr_count_opaque(_ptr(_f32c(rays)), _ptr(_f32c(depth_gt)), rays.shape[0], _ptr(n_rays_dev), _ptr(far0),
                                  _ptr(counts), _stream()), "lnr_count_opaque")
    return counts


def los_loss_fused(sigma, z, rays, depth_gt, scale, cfg: hip.LossConfig, counts, noise=None, noise_std=0.0, seed=0,
                   n_rays_dev=None, want_stats=False, want_weights=False, loss_out=None, far0=None, poison=None, poison_tag=0,
                   zero_dead_rows=True):
    """zero_dead_rows=False: d_rays rows at and beyond *n_rays_dev are left uninitialised (the kernel writes every column of every live
    row; the training loop never reads the others and saves a fill launch per iteration)."""
    require_device(sigma, z, rays, depth_gt, counts, noise, far0, poison)
    sigma, z, rays, depth_gt = _f32c(sigma), _f32c(z), _f32c(rays), _f32c(depth_gt)
    n, s = z.shape
    dev = z.device
    if loss_out is None:
        loss_out = torch.zeros(8, device=dev)
    d_sigma = torch.empty(n, s, device=dev)
    d_rays = (torch.zeros if (zero_dead_rows and n_rays_dev is not None) else torch.empty)(n, hip.RAY_STRIDE, device=dev)
    stats = torch.zeros(n, 8, device=dev) if want_stats else None
    w = torch.zeros(n, s, device=dev) if want_weights else None
    partials = torch.empty(((n + hip.LOSS_RAYS_PER_BLOCK - 1) // hip.LOSS_RAYS_PER_BLOCK) * 8, device=dev)
    check(load().lnr_los_loss_fused(_ptr(sigma), _ptr(z), _ptr(rays), _ptr(depth_gt), n, _ptr(n_rays_dev), s,
                                    _ptr(_f32c(noise)), float(noise_std), int(seed), float(scale), C.byref(cfg), _ptr(counts),
                                    _ptr(far0), _ptr(loss_out), _ptr(d_sigma), _ptr(d_rays), _ptr(stats), _ptr(w), _ptr(partials),
                                    _ptr(poison), int(poison_tag), _stream()),
          "lnr_los_loss_fused")
    return loss_out, d_sigma, d_rays, stats, w


# ---------------------------------------------------------------- optimisers
def adam_step(params, grads, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=True, poison=None):
    require_device(params, grads, exp_avg, exp_avg_sq, poison)
    check(load().lnr_adam_step(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), float(lr),
                               float(betas[0]), float(betas[1]), float(eps), int(step), float(grad_scale), int(zero_grad),
                               _ptr(poison), _stream()), "lnr_adam_step")


def occ_grid_step(grid, rays, z, depth_gt, scale, lr, margin=2.0, l_free=0.25, l_occ=2.5, grad_buf=None, n_rays_dev=None):
    """grad_buf: int64 [V^3] fixed-point accumulator (see the header) or None for the in-place float-atomic update."""
    require_device(grid, rays, z, depth_gt, grad_buf)
    assert grad_buf is None or (grad_buf.dtype == torch.int64 and grad_buf.is_contiguous())
    v = grid.shape[-1]
    n, s = z.shape
    check(load().lnr_occ_grid_step(_ptr(grid), v, _ptr(_f32c(rays)), _ptr(_f32c(z)), _ptr(_f32c(depth_gt)), n, _ptr(n_rays_dev),
                                   s, float(scale), float(lr), float(margin), float(l_free), float(l_occ), _ptr(grad_buf),
                                   _stream()), "lnr_occ_grid_step")


def occ_grid_apply(grid, grad_buf, lr, zero_grad=True, poison=None):
    require_device(grid, grad_buf, poison)
    assert grad_buf.dtype == torch.int64 and grad_buf.is_contiguous()
    check(load().lnr_occ_grid_apply(_ptr(grid), _ptr(grad_buf), grid.numel(), float(lr), int(zero_grad), _ptr(poison), _stream()),
          "lnr_occ_grid_apply")


def rng_draws(which, seed, n_rays, n_per_ray, device="cuda"):
    """The in-kernel generator's draws as a tensor [n_rays, n_per_ray] (hip.DRAW_JITTER / DRAW_PDF / DRAW_NOISE / DRAW_RAY_INDEX + segment)."""
    out = torch.empty(int(n_rays), int(n_per_ray), device=device, dtype=torch.float32)
    check(load().lnr_rng_draws(int(which), int(seed) & (2 ** 64 - 1), int(n_rays), int(n_per_ray), _ptr(out), _stream()), "lnr_rng_draws")
    return out


def selftest_mfma(device="cuda"):
    """max abs error of the three MFMA fragment-layout checks (fp32 16x16x4, fp16 16x16x32, the three-term bf16 split on 16x16x32);
    0.0 when all layouts hold (and the split product of the test operands is exact)."""
    out = torch.full((3,), -1.0, device=device)
    check(load().lnr_selftest_mfma(_ptr(out), _stream()), "lnr_selftest_mfma")
    return float(out.abs().max().item()) if bool((out >= 0).all()) else -1.0
