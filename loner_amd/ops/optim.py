"""Parameter updates and self-checks: Adam, the occupancy grid's step and apply, the generator's draws, the MFMA layout test.
Mapping loop (adam_step, occ_grid_step, occ_grid_apply): caller-owned fp32 tensors updated in place, nothing allocated, nothing read
back, wrong dtypes are assertions.  rng_draws and selftest_mfma are test hooks; selftest_mfma reads its result back."""
import torch

from ..hip import _ptr, _stream, check, load, require_device
from ._common import _U64, _f32c


def adam_step(params, grads, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, zero_grad=True, poison=None):
    require_device(params, grads, exp_avg, exp_avg_sq, poison)
    check(load().lnr_adam_step(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), float(lr), float(betas[0]), float(betas[1]),
                               float(eps), int(step), float(grad_scale), int(zero_grad), _ptr(poison), _stream()), "lnr_adam_step")


def occ_grid_step(grid, rays, z, depth_gt, scale, lr, margin=2.0, l_free=0.25, l_occ=2.5, grad_buf=None, n_rays_dev=None):
    """grad_buf: int64 [V^3] fixed-point accumulator (see the header) or None for the in-place float-atomic update."""
    require_device(grid, rays, z, depth_gt, grad_buf)
    assert grad_buf is None or (grad_buf.dtype == torch.int64 and grad_buf.is_contiguous())
    v = grid.shape[-1]
    n, s = z.shape
    check(load().lnr_occ_grid_step(_ptr(grid), v, _ptr(_f32c(rays)), _ptr(_f32c(z)), _ptr(_f32c(depth_gt)), n, _ptr(n_rays_dev), s, float(scale), float(lr),
                                   float(margin), float(l_free), float(l_occ), _ptr(grad_buf), _stream()), "lnr_occ_grid_step")


def occ_grid_apply(grid, grad_buf, lr, zero_grad=True, poison=None):
    require_device(grid, grad_buf, poison)
    assert grad_buf.dtype == torch.int64 and grad_buf.is_contiguous()
    check(load().lnr_occ_grid_apply(_ptr(grid), _ptr(grad_buf), grid.numel(), float(lr), int(zero_grad), _ptr(poison), _stream()), "lnr_occ_grid_apply")


def rng_draws(which, seed, n_rays, n_per_ray, device="cuda"):
    """The in-kernel generator's draws as a tensor [n_rays, n_per_ray] (hip.DRAW_JITTER / DRAW_PDF / DRAW_NOISE / DRAW_RAY_INDEX + segment)."""
    out = torch.empty(int(n_rays), int(n_per_ray), device=device, dtype=torch.float32)
    check(load().lnr_rng_draws(int(which), int(seed) & _U64, int(n_rays), int(n_per_ray), _ptr(out), _stream()), "lnr_rng_draws")
    return out


def selftest_mfma(device="cuda"):
    """max abs error of the three MFMA fragment-layout checks (fp32 16x16x4, fp16 16x16x32, the three-term bf16 split on 16x16x32);
    0.0 when all layouts hold (and the split product of the test operands is exact)."""
    out = torch.full((3,), -1.0, device=device)
    check(load().lnr_selftest_mfma(_ptr(out), _stream()), "lnr_selftest_mfma")
    return float(out.abs().max().item()) if bool((out >= 0).all()) else -1.0
