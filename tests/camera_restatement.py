"""CPU restatement of the camera renderer's contract (include/loner_hip.h: lnr_build_camera_rays, lnr_render_forward_peak,
lnr_depth_colormap; loner_amd/analysis/renderer.py): the ray records in torch fp32, the peak in torch, the colour map in numpy fp32,
the OpenCV distortion model, a PNG decoder, and the fly-through written on scipy from its description."""
import os
import struct
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_camera_rays.npz")))


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ---------------------------------------------------------------- ray records
def camera_rays(directions, index, width, T, range_min, scale, shift):
    """fp32 torch on the CPU, every operation on its own: the record of include/loner_hip.h (lnr_build_camera_rays).  directions
    [n_pixels,3], index int64 [n] or None, T [3,4] or [4,4], shift [3]."""
    f = lambda x: torch.as_tensor(x, dtype=torch.float32)
    directions, T, shift, scale = f(directions), f(T), f(shift).reshape(3), f(scale)
    index = torch.arange(directions.shape[0]) if index is None else torch.as_tensor(index, dtype=torch.int64)
    d = directions[index]
    R = T[:3, :3]
    v = (R[None, :, 0] * d[:, 0:1] + R[None, :, 1] * d[:, 1:2]) + R[None, :, 2] * d[:, 2:3]
    nrm = torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    dirs = v / nrm[:, None]
    o = ((T[:3, 3] + shift) / scale)[None, :].expand(d.shape[0], 3)
    dd = dirs + 1e-15
    far = torch.maximum(((-1.0 - o) / dd).clamp(min=0), ((1.0 - o) / dd).clamp(min=0)).min(dim=1, keepdim=True).values
    near = (f(range_min) / scale) * torch.ones_like(far)
    x = (index % width).float()[:, None]
    y = torch.div(index, width, rounding_mode="floor").float()[:, None]
    return torch.cat([o, dirs, -dirs, x, y, near, far], dim=1)


# ---------------------------------------------------------------- distortion
def distort_points(points, k, distortion):
    """The OpenCV plumb-bob model forwards, fp64: undistorted NORMALISED coordinates [n,2] -> pixels of the distorted image with k."""
    d = np.zeros(5)
    d[:len(distortion)] = distortion
    k1, k2, p1, p2, k3 = d
    x, y = points[:, 0], points[:, 1]
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([k[0, 0] * xd + k[0, 2], k[1, 1] * yd + k[1, 2]], axis=1)


# ---------------------------------------------------------------- peak
def peak(weights, z):
    """(peak_z, peak_index): torch.argmax's rules on the CPU - the first of equal maxima, a NaN counts as maximal"""
    w = torch.as_tensor(weights).cpu()
    idx = w.argmax(dim=1)
    return torch.as_tensor(z).cpu()[torch.arange(w.shape[0]), idx], idx


# ---------------------------------------------------------------- colour map
def depth_colormap(values, table, multiplier=1.0, min_depth=1, max_depth=50):
    """numpy fp32, step by step as include/loner_hip.h states lnr_depth_colormap (= save_depth, analysis/render_utils.py:116-127 of
    the reference, with matplotlib's index rule and the truncating * 255 -> uint8 folded into `table` uint8 [256,3])."""
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(values, dtype=f32) * f32(multiplier)).astype(f32)
        lo, hi, span = f32(min_depth), f32(max_depth), f32(float(max_depth) - float(min_depth))
        mask = v >= hi
        c = np.minimum(np.maximum(v, lo), hi)
        x = ((c - lo).astype(f32) / span).astype(f32)
        x = np.minimum(np.maximum(x, f32(0)), f32(1))
        bad = np.isnan(x)
        k = np.minimum(np.floor(np.where(bad, f32(0), x) * f32(256)), 255).astype(np.int64)
    out = np.empty(v.shape + (4,), dtype=np.uint8)
    out[..., :3] = np.asarray(table, dtype=np.uint8)[k]
    out[..., 3] = 255
    out[mask] = (0, 0, 0, 255)
    out[bad] = (0, 0, 0, 0)
    return out


COLOUR_SPECIALS = [float("nan"), float("inf"), float("-inf"), 1.0, 50.0, 49.999996, 0.0, -3.0, 1e30] + \
                  [1.0 + 49.0 * k / 256 for k in (1, 2, 127, 128, 255)]


def colour_image(h=37, w=53, seed=4):
    """fp32 [h,w] metres in about [-5, 60] with COLOUR_SPECIALS planted at the start"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-5.0, 60.0, size=(h, w)).astype(np.float32)
    img.reshape(-1)[:len(COLOUR_SPECIALS)] = np.asarray(COLOUR_SPECIALS, dtype=np.float32)
    return img


# ---------------------------------------------------------------- PNG
def read_png(path):
    """uint8 [H,W,channels] of an 8-bit, non-interlaced PNG: chunks and CRCs checked, every filter type undone"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(tag + body) & 0xFFFFFFFF), tag
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert tag == b"IEND"
    w, h, depth, colour, comp, filt, lace = head
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    ch = {0: 1, 2: 3, 6: 4}[colour]
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), dtype=np.uint8)
    for r in range(h):
        ft, line = int(raw[r, 0]), raw[r, 1:].astype(np.int64)
        up = out[r - 1].astype(np.int64) if r else np.zeros(w * ch, dtype=np.int64)
        if ft == 0:
            rec = line
        elif ft == 2:
            rec = line + up
        else:
            rec = np.zeros(w * ch, dtype=np.int64)
            for i in range(w * ch):
                a = rec[i - ch] if i >= ch else 0
                b = up[i]
                c = up[i - ch] if i >= ch else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                rec[i] = (line[i] + p) & 255
        out[r] = (rec & 255).astype(np.uint8)
    return out.reshape(h, w, ch)


# ---------------------------------------------------------------- fly-through
def trajectory_rows(n=30, length=25.0, seed=2):
    """TUM rows [n,8]: a gently turning, climbing path `length` metres long with rotations that move with it"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, n)
    xyz = np.stack([length * 0.9 * s + 2.0, 3.0 * np.sin(3.0 * s) - 1.0, 0.5 * s + 0.2 * np.cos(5 * s)], axis=1)
    seg = np.sqrt((np.diff(xyz, axis=0) ** 2).sum(1)).sum()
    xyz = xyz[0] + (xyz - xyz[0]) * (length / seg)
    rot = Rotation.from_euler("ZYX", np.stack([1.4 * s + 0.3, 0.2 * np.sin(4 * s), 0.1 * s], axis=1) + 0.01 * rng.normal(size=(n, 3)))
    return np.concatenate([np.arange(n, dtype=np.float64)[:, None] * 0.1, xyz, rot.as_quat()], axis=1)


def flythrough_reference(rows, velocity=1.0, fps=5, spin_spacing_m=10.0, spin_duration_s=15.0, render_global=False, interpolate=True):
    """The fly-through as loner_amd/analysis/renderer.py describes it, written on scipy -> (poses fp64 [n,4,4], spin_idxs).
    Time is arc length / velocity; int(duration * fps) images are spread evenly over it, rotations by scipy's Slerp and positions by
    interp1d, all at once.  Then one walk adds the spins: the distance travelled grows by the step from the last position (the
    origin before the first image), and once it exceeds the spacing the camera turns about its own z in int(spin_duration_s * fps)
    steps from 0 to 2 pi, each spin pose's index listed twice, and the distance starts again."""
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp
    rows = np.asarray(rows, dtype=np.float64)

    def homogeneous(R, p):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, p
        return M

    world = np.stack([homogeneous(R, p) for R, p in zip(Rotation.from_quat(rows[:, 4:]).as_matrix(), rows[:, 1:4])])
    if not render_global:
        world = np.linalg.inv(world[0]) @ world
    if not interpolate:
        return world, []
    positions = world[:, :3, 3]
    arc = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(positions, axis=0), axis=1))]) / velocity
    at = np.linspace(0.0, arc[-1], int(arc[-1] * fps))
    Rs = Slerp(arc, Rotation.from_matrix(world[:, :3, :3]))(at).as_matrix()
    ps = interp1d(arc, positions, axis=0)(at)
    turn = Rotation.from_euler("z", np.linspace(0.0, 2.0 * np.pi, int(spin_duration_s * fps))).as_matrix()
    poses, spin_idxs, travelled, last = [], [], 0.0, np.zeros(3)
    for R, p in zip(Rs, ps):
        poses.append(homogeneous(R, p))
        travelled += float(np.linalg.norm(p - last))
        last = p
        if travelled > spin_spacing_m:
            for Rz in turn:
                spin_idxs += [len(poses), len(poses)]
                poses.append(homogeneous(R @ Rz, p))
            travelled = 0.0
    return np.stack(poses), spin_idxs
