"""The density network: workspace, route, forward, backward, weight-gradient fold, the per-kernel profile hooks.
Mapping loop, every iteration: fp32 device tensors (other float dtypes are converted); the device is read back only where the
workspace grows and in density_clipped_count.  A caller-owned output of the wrong dtype or shape is an assertion; RuntimeError: the
library refused the call, or reuse_features named another forward."""
import ctypes as C

import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _f32c


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


_workspaces = {}


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


def density_forward(spec, params, pts=None, rays=None, z=None, n_rays_dev=None, forward_only=False, out=None):
    """forward_only: the caller will not call density_backward(reuse_features=True) on these points - the workspace is sized
    for the forward alone (rendering / inference: no record regions).
    out: a contiguous float32 tensor of the result's shape to write sigma into instead of a new one (rays form: the rows from
    *n_rays_dev on keep what they held)."""
    require_device(params, pts, rays, z)
    params = _f32c(params)
    if pts is not None:                                 # the points form: rays, z and n_rays_dev stay out of the call
        pts = _f32c(pts).reshape(-1, 3)
        n_pts, n, s, rays, z, n_rays_dev = pts.shape[0], 0, 0, None, None, None
        shape, features_of = (n_pts,), (params.data_ptr(), pts.data_ptr(), 0, n_pts)
    else:                                               # the rays form
        rays, z = _f32c(rays), _f32c(z)
        n_pts, (n, s) = 0, z.shape
        shape, features_of = (n, s), (params.data_ptr(), rays.data_ptr(), z.data_ptr(), n * s)
    ent, need = _workspace(spec, params.device, features_of[3], forward_only)
    assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape and out.device == params.device)
    sigma = torch.empty(*shape, device=params.device, dtype=torch.float32) if out is None else out      # (rays form: rows >= *n_rays_dev stay unread)
    check(load().lnr_density_forward(C.byref(spec), _ptr(params), _ptr(pts), n_pts, _ptr(rays), _ptr(z), n, s, _ptr(n_rays_dev), _ptr(sigma),
                                     _ptr(ent["buf"]), need, _stream()), "lnr_density_forward")
    ent["features_of"] = None if forward_only else features_of
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
                     want_d_pts=False, reuse_features=False, d_rays=None, table_atomics=False, report_regions=False, input_grad_event=None,
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
        (hip.BWD_DEFER_WEIGHT_FOLD if defer_weight_fold else 0) | (hip.BWD_OVERWRITE_GRAD if overwrite_grad else 0)
    if pts is not None:                                 # the points form: rays, z and n_rays_dev stay out of the call
        pts = _f32c(pts).reshape(-1, 3)
        n_pts, n, s, rays, z, n_rays_dev, d_rays = pts.shape[0], 0, 0, None, None, None, None
        shape, features_of = (n_pts,), (params.data_ptr(), pts.data_ptr(), 0, n_pts)
    else:                                               # the rays form
        rays, z = _f32c(rays), _f32c(z)
        n_pts, (n, s) = 0, z.shape
        shape, features_of = (n, s), (params.data_ptr(), rays.data_ptr(), z.data_ptr(), n * s)
    ent, need = _workspace(spec, params.device, features_of[3])
    reuse = int(bool(reuse_features))
    if reuse and ent["features_of"] != features_of:
        raise RuntimeError("density_backward(reuse_features=True): workspace features belong to a different forward call")
    d_pts = torch.empty(*shape, 3, device=params.device, dtype=torch.float32) if want_d_pts else None
    check(load().lnr_density_backward(C.byref(spec), _ptr(params), _ptr(pts), n_pts, _ptr(rays), _ptr(z), n, s, _ptr(n_rays_dev),
                                      _ptr(d_sigma), _ptr(grad_params), _ptr(d_pts), _ptr(d_rays), reuse, flags, _ptr(ent["buf"]), need,
                                      _event(input_grad_event), _stream()), "lnr_density_backward")
    return d_pts


def density_fold_weight_grads(spec, grad_params, n_points, overwrite_grad=False):
    """Adds the weight-gradient slabs a density_backward(defer_weight_fold=True) call left in the workspace to grad_params
    (on the current stream: the training loop does it on its side stream, beside the table-gradient reduce)."""
    require_device(grad_params)
    ent, need = _workspace(spec, grad_params.device, n_points)
    check(load().lnr_density_fold_weight_grads(C.byref(spec), int(n_points), _ptr(grad_params), _ptr(ent["buf"]), need,
                                               hip.BWD_OVERWRITE_GRAD if overwrite_grad else 0, _stream()),
          "lnr_density_fold_weight_grads")
