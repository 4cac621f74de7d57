"""Plumbing every ops module shares: input coercion, status words, scratch buffers, small ctypes literals.  Nothing here belongs to
one family of entry points or launches a kernel; the helpers that raise keep their callers' message text (the tests match it)."""
import ctypes as C
import math

import torch

from ..hip import require_device

_U64 = 2 ** 64 - 1                      # seeds reach the library as uint64: int(seed) & _U64
_held = {}                              # _held_buffer: (name, device) -> tensor


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _float3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


def _positive(value, what, name):
    v = float(value)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{what}: {name} must be finite and > 0, got {value!r}")
    return v


def _render_inputs(sigma, z, rays):
    """-> (sigma, z, rays as contiguous fp32, n rays, samples per ray)"""
    z = _f32c(z)
    return _f32c(sigma), z, _f32c(rays), z.shape[0], z.shape[1]


def _f64_points(t, what):
    require_device(t)
    assert t.dim() == 2 and t.shape[1] == 3, f"{what}: points [n,3]"
    return t.to(torch.float64).contiguous()


def _mesh_triangles(triangles, what):
    require_device(triangles)
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int32:
        raise ValueError(f"{what}: triangles int32 [F,3], got {tuple(triangles.shape)} {triangles.dtype}")
    return triangles.contiguous()


def _float_rows(t, width, what, name):
    """ValueError unless t is a tensor [n,width] of a float dtype: the [n,6] rays and [n,3] points of the BVH walks and the TSDF"""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != width or not t.dtype.is_floating_point:
        raise ValueError(f"{what}: {name} [n,{width}] of a float dtype, got {tuple(getattr(t, 'shape', ()))} "
                         f"{getattr(t, 'dtype', type(t).__name__)}")


def _raise_status(what, status, messages, lead=""):
    """RuntimeError that names every set bit of a call's status word (`lead` goes before the names); nothing when it is 0"""
    if status:
        raise RuntimeError(f"{what}: {lead}" + ", ".join(m for b, m in messages.items() if status & b))


def _scratch(need, device, over_limit=None, held=None):
    """(uint8 buffer, bytes) for a size the library reported; 0 means the input is over the library's limit: RuntimeError(over_limit),
    where the caller gives one.  A buffer per call (the caching allocator's, so calls on different streams never share one), or with
    held (a name) the buffer kept under that name for the device, grown on demand: calls on one stream reuse it in order."""
    need = int(need)
    if need == 0 and over_limit is not None:
        raise RuntimeError(over_limit)
    if held is None:
        return torch.empty(need, device=device, dtype=torch.uint8), need
    return _held_buffer(held, device, need), need


def _held_buffer(name, device, count, dtype=torch.uint8):
    """The buffer kept under `name` for `device`, replaced by a larger one when it has fewer than `count` elements"""
    key = (name, str(device))
    buf = _held.get(key)
    if buf is None or buf.numel() < count:
        _held.pop(key, None)                        # the old buffer goes before the larger one is allocated
        buf = _held[key] = torch.empty(count, device=device, dtype=dtype)
    return buf
