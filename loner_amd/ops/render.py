"""Sampling, volume rendering and the loss: samplers, render forward / peak / backward / front-to-back, colormap, loss pieces.
Mapping loop and inference: fp32 device tensors (other float dtypes are converted), never a read back.  Wrong dtypes or shapes are
assertions, a bad scalar is a ValueError; RuntimeError: a tensor is not on the device, or the library refused."""
import ctypes as C

import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _U64, _f32c, _render_inputs

_steps_cache = {}


def linspace_table(count: int, device) -> torch.Tensor:
    """torch.linspace(0,1,count) on `device` (ray_sampling.py:27,59); cached."""
    key = (count, str(device))
    t = _steps_cache.get(key)
    if t is None:
        t = torch.linspace(0, 1, count).to(device)
        _steps_cache[key] = t
    return t


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
    check(load().lnr_sample_rays_occ(_ptr(rays), n, _ptr(n_rays_dev), _ptr(g), v, n_samples, float(perturb), _ptr(steps), _ptr(_f32c(u_jitter)),
                                     _ptr(_f32c(u_pdf)), int(seed) & _U64, _ptr(z), _ptr(inds), _ptr(probs), _ptr(cdf), _stream()), "lnr_sample_rays_occ")
    if debug:
        return z, dict(inds=inds, probs=probs, cdf=cdf)
    return z


def sample_rays_uniform(rays, n_samples, perturb, u_jitter=None, seed=0, n_rays_dev=None):
    require_device(rays, u_jitter)
    rays = _f32c(rays)
    n = rays.shape[0]
    steps = linspace_table(n_samples, rays.device)
    z = torch.zeros(n, n_samples, device=rays.device, dtype=torch.float32)
    check(load().lnr_sample_rays_uniform(_ptr(rays), n, _ptr(n_rays_dev), n_samples, float(perturb), _ptr(steps), _ptr(_f32c(u_jitter)), int(seed) & _U64,
                                         _ptr(z), _stream()), "lnr_sample_rays_uniform")
    return z


def ftb_gather(rays, z, idx, n_alive, b0, block, rays_c, z_c, next_count):
    """front-to-back inference (lnr_render_ftb_gather): alive rays' records and block depths -> the compact arrays rays_c / z_c"""
    require_device(rays, z, idx, n_alive, rays_c, z_c, next_count)
    check(load().lnr_render_ftb_gather(_ptr(rays), _ptr(z), z.shape[1], _ptr(idx), _ptr(n_alive), rays.shape[0], int(b0), int(block), _ptr(rays_c),
                                       _ptr(z_c), _ptr(next_count), _stream()), "lnr_render_ftb_gather")


def ftb_composite(sigma_c, z, rays, idx, n_alive, b0, block, noise_std, seed, transmittance, depth_acc, opacity_acc, next_idx, next_count, last, noise=None):
    """front-to-back inference (lnr_render_ftb_composite): one block's contributions of the alive rays; survivors appended to next_idx"""
    require_device(sigma_c, z, rays, idx, n_alive, transmittance, depth_acc, opacity_acc, next_idx, next_count, noise)
    check(load().lnr_render_ftb_composite(_ptr(sigma_c), _ptr(z), _ptr(rays), z.shape[1], _ptr(idx), _ptr(n_alive), rays.shape[0], int(b0), int(block),
                                          _ptr(_f32c(noise) if noise is not None else None), float(noise_std), int(seed), _ptr(transmittance),
                                          _ptr(depth_acc), _ptr(opacity_acc), _ptr(next_idx), _ptr(next_count), 1 if last else 0,
                                          _stream()), "lnr_render_ftb_composite")


def render_forward(sigma, z, rays, noise=None, noise_std=0.0, seed=0, n_rays_dev=None, want_weights=True):
    """-> (depth, weights, opacity, variance); want_weights=False leaves the [n, S] weights unwritten (returns None for them)."""
    require_device(sigma, z, rays, noise)
    sigma, z, rays, n, s = _render_inputs(sigma, z, rays)
    dev = z.device
    depth, opacity, variance = (torch.zeros(n, device=dev) for _ in range(3))
    weights = torch.zeros(n, s, device=dev) if want_weights else None
    check(load().lnr_render_forward(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)), float(noise_std), int(seed), _ptr(depth),
                                    _ptr(weights), _ptr(opacity), _ptr(variance), _stream()), "lnr_render_forward")
    return depth, weights, opacity, variance


def render_forward_peak(sigma, z, rays, noise=None, noise_std=0.0, seed=0, n_rays_dev=None):
    """-> (depth, opacity, variance, peak_z, peak_index int32): render_forward's depth, opacity and variance bit for bit, and per ray
    the sample of maximal weight (torch.argmax's rules) with its depth - no [n, S] weights (lnr_render_forward_peak)."""
    require_device(sigma, z, rays, noise)
    sigma, z, rays, n, s = _render_inputs(sigma, z, rays)
    dev = z.device
    depth, opacity, variance, peak_z = (torch.zeros(n, device=dev) for _ in range(4))
    peak_index = torch.zeros(n, device=dev, dtype=torch.int32)
    check(load().lnr_render_forward_peak(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)), float(noise_std), int(seed),
                                         _ptr(depth), _ptr(opacity), _ptr(variance), _ptr(peak_z), _ptr(peak_index), _stream()), "lnr_render_forward_peak")
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
    check(load().lnr_depth_colormap(_ptr(values), values.numel(), float(multiplier), float(min_depth), float(max_depth), _ptr(table), _ptr(rgba),
                                    _stream()), "lnr_depth_colormap")
    return rgba


def render_backward(sigma, z, rays, g_depth, g_weights, g_opacity, g_variance, noise=None, noise_std=0.0, seed=0,
                    n_rays_dev=None):
    require_device(sigma, z, rays)
    sigma, z, rays, n, s = _render_inputs(sigma, z, rays)
    d_sigma = torch.zeros(n, s, device=z.device)
    d_rays = torch.zeros(n, hip.RAY_STRIDE, device=z.device)
    check(load().lnr_render_backward(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)), float(noise_std), int(seed),
                                     _ptr(_f32c(g_depth)), _ptr(_f32c(g_weights)), _ptr(_f32c(g_opacity)), _ptr(_f32c(g_variance)), _ptr(d_sigma),
                                     _ptr(d_rays), _stream()), "lnr_render_backward")
    return d_sigma, d_rays


def points_grad_to_rays(d_pts, z, d_rays, n_rays_dev=None):
    require_device(d_pts, z, d_rays)
    n, s = z.shape
    check(load().lnr_points_grad_to_rays(_ptr(_f32c(d_pts)), _ptr(_f32c(z)), n, _ptr(n_rays_dev), s, _ptr(d_rays), _stream()), "lnr_points_grad_to_rays")
    return d_rays


def weights_gt(s, g, eps, normalise=True):
    require_device(s, g)
    s = _f32c(s)
    n, k = s.shape
    g = _f32c(g).reshape(-1)
    out = torch.empty_like(s)
    e = None                                            # eps: one number, or a tensor with one per row
    if isinstance(eps, torch.Tensor):
        require_device(eps)
        e = _f32c(eps).reshape(-1)
    check(load().lnr_weights_gt(_ptr(s), _ptr(g), _ptr(e), 0.0 if e is not None else float(eps), int(normalise), n, k, _ptr(out),
                                _stream()), "lnr_weights_gt")
    return out


def logits_grad(s, g, margin=2.0, l_free=0.25, l_occ=2.5):
    require_device(s, g)
    s = _f32c(s)
    n, k = s.shape
    out = torch.empty_like(s)
    check(load().lnr_logits_grad(_ptr(s), _ptr(_f32c(g).reshape(-1)), n, k, float(margin), float(l_free), float(l_occ), _ptr(out),
                                 _stream()), "lnr_logits_grad")
    return out


def count_opaque(rays, depth_gt, n_rays_dev=None, far0=None):
    """-> int32 [2] = {#rays, #opaque rays}.  far0 (device float [1], optional): the `far` every depth is compared with
    (the reference's far[0] quirk) when `rays` is only a shard of the batch."""
    require_device(rays, depth_gt, far0)
    counts = torch.empty(2, device=rays.device, dtype=torch.int32)       # overwritten, also for an empty batch
    check(load().lnr_count_opaque(_ptr(_f32c(rays)), _ptr(_f32c(depth_gt)), rays.shape[0], _ptr(n_rays_dev), _ptr(far0), _ptr(counts),
                                  _stream()), "lnr_count_opaque")
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
    check(load().lnr_los_loss_fused(_ptr(sigma), _ptr(z), _ptr(rays), _ptr(depth_gt), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)), float(noise_std),
                                    int(seed), float(scale), C.byref(cfg), _ptr(counts), _ptr(far0), _ptr(loss_out), _ptr(d_sigma), _ptr(d_rays),
                                    _ptr(stats), _ptr(w), _ptr(partials), _ptr(poison), int(poison_tag), _stream()), "lnr_los_loss_fused")
    return loss_out, d_sigma, d_rays, stats, w
