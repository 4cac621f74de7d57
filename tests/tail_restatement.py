"""Dtype-generic restatement of the pose-gradient tail and of the update kernels (include/loner_hip.h: lnr_pose_forward / backward,
lnr_build_window_rays, lnr_lidar_rays_backward, lnr_points_grad_to_rays, lnr_adam_step, lnr_occ_grid_step / apply).

Plain torch, no casts: every function computes in the dtype of what it is given, so the same code is the truth in float64 and the
noise yardstick in float32 (`block_err`, `bound`).  Gradients come from autograd.  Nothing here calls oracle/: tests/test_tail_host.py
ties the float32 run to it and the float64 run to central finite differences."""
import math

import torch

F32_EPS = 2.0 ** -23
RAY_STRIDE = 13


# ---------------------------------------------------------------- yardstick
def block_err(x, ref):
    """largest absolute deviation of a block from its float64 reference"""
    if ref.numel() == 0:
        return 0.0
    return float((x.detach().cpu().double() - ref.detach().cpu().double()).abs().max())


def block_max(ref):
    return float(ref.detach().abs().max()) if ref.numel() else 0.0


def bound(noise, ref):
    """4 x (error of the float32 restatement on the same block) + 4 ulp of the block's largest reference entry"""
    return 4.0 * noise + 4.0 * F32_EPS * block_max(ref)


def elementwise_rel(x, ref, floor):
    """max_i |x_i - ref_i| / max(|ref_i|, floor_i); floor: a number, or per element the size of the terms the element is the sum of"""
    if ref.numel() == 0:
        return 0.0
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    return float(((x - ref).abs() / torch.maximum(ref.abs(), torch.as_tensor(floor, dtype=torch.float64))).max())


# ---------------------------------------------------------------- pose6 -> [R|t]
def skew(aa):
    zero = torch.zeros_like(aa[..., 0])
    a, b, c = aa.unbind(-1)
    return torch.stack([zero, -c, b, c, zero, -a, -b, a, zero], dim=-1).reshape(aa.shape[:-1] + (3, 3))


def rotation_quat(aa):
    """the quaternion form of oracle/poses.py (pytorch3d's axis_angle_to_matrix): series for sin(h)/theta below 1e-6 rad"""
    theta = torch.linalg.vector_norm(aa, dim=-1, keepdim=True)
    half = 0.5 * theta
    tiny = theta.abs() < 1e-6
    safe = torch.where(tiny, torch.ones_like(theta), theta)
    k = torch.where(tiny, 0.5 - theta * theta / 48.0, torch.sin(half) / safe)
    q = torch.cat([torch.cos(half), aa * k], dim=-1)
    w, x, y, z = q.unbind(-1)
    s2 = 2.0 / (q * q).sum(-1)
    rows = torch.stack([1 - s2 * (y * y + z * z), s2 * (x * y - z * w), s2 * (x * z + y * w),
                        s2 * (x * y + z * w), 1 - s2 * (x * x + z * z), s2 * (y * z - x * w),
                        s2 * (x * z - y * w), s2 * (y * z + x * w), 1 - s2 * (x * x + y * y)], dim=-1)
    return rows.reshape(aa.shape[:-1] + (3, 3))


def rotation_exp(aa):
    """exp of the skew matrix: knows nothing of quaternions or of the series switch"""
    return torch.linalg.matrix_exp(skew(aa))


def transforms(pose6, form="exp"):
    """pose6 [n,6] = [t, axis-angle] -> [R|t] [n,3,4]"""
    R = rotation_exp(pose6[:, 3:6]) if form == "exp" else rotation_quat(pose6[:, 3:6])
    return torch.cat([R, pose6[:, 0:3, None]], dim=2)


# ---------------------------------------------------------------- [R|t] -> ray records
def per_axis_exit(origins, dirs):
    """[m,3]: per axis the larger of the two clamped plane distances of the cube [-1,1]^3, direction offset by 1e-15"""
    d = dirs + 1e-15
    t_lo = ((-1.0 - origins) / d).clamp(min=0)
    t_hi = ((1.0 - origins) / d).clamp(min=0)
    return torch.maximum(t_lo, t_hi)


def ray_records(T, directions, index, ray_range, scale, shift):
    """T [3,4] (lidar -> world), directions [3,n] sensor frame, index [m] -> records [m,13] =
    [origin(3) dir(3) viewdir(3) 0 0 near far]; far = min(range_max / scale, cube exit).  R l is the plain product."""
    m = index.shape[0]
    local = directions[:, index]
    origin = (T[:, 3] + shift) / scale
    origins = origin[None, :].expand(m, 3)
    world = (T[:, :3] @ local).T
    unit = world / torch.linalg.vector_norm(world, dim=1, keepdim=True)
    ones = torch.ones_like(unit[:, :1])
    near = ray_range[0] / scale * ones
    far_range = ray_range[1] / scale * ones
    far = torch.minimum(far_range, per_axis_exit(origins, unit).min(dim=1, keepdim=True).values)
    return torch.cat([origins, unit, -unit, torch.zeros_like(unit[:, :2]), near, far], dim=1)


def near_tie(rays, far_range, rel=1e-3):
    """rays whose far an fp32 evaluation may legitimately take from another plane than fp64 does: the two smallest per-axis
    exits, or the cube exit and the range limit, lie within `rel` of each other"""
    ex = per_axis_exit(rays[:, 0:3], rays[:, 3:6]).sort(dim=1).values
    two = (ex[:, 1] - ex[:, 0]) < rel * ex[:, 1]
    rng = (ex[:, 0] - far_range).abs() < rel * far_range
    return two | rng


def exit_face(rays, far_range):
    """0..5 = -x +x -y +y -z +z for rays that end on the cube, -1 for range-limited rays"""
    ex = per_axis_exit(rays[:, 0:3], rays[:, 3:6])
    t, axis = ex.min(dim=1)
    sign = (rays[:, 3:6].gather(1, axis[:, None])[:, 0] > 0).long()
    return torch.where(t < far_range, 2 * axis + sign, torch.full_like(axis, -1))


# ---------------------------------------------------------------- d_pts -> d_rays[:, 0:6]
def points_grad_to_rays(d_pts, z):
    """p = o + d z:  dL/do = sum_s g,  dL/dd = sum_s z g;  d_pts [n,S,3], z [n,S] -> [n,6]"""
    return torch.cat([d_pts.sum(dim=1), (z[..., None] * d_pts).sum(dim=1)], dim=1)


def chain_loss_terms(p):
    """sum over samples of sin(3x) + cos(2y) z + 0.5 x y"""
    x, y, z = p.unbind(-1)
    return (torch.sin(3.0 * x) + torch.cos(2.0 * y) * z + 0.5 * x * y).sum()


# ---------------------------------------------------------------- Adam
def adam_step(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """torch.optim.Adam (no weight decay, no amsgrad) on grad_scale * g -> (p, m, v), new tensors"""
    c1 = 1.0 - b1 ** step
    c2 = math.sqrt(1.0 - b2 ** step)
    gg = g * grad_scale
    m = m + (gg - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * gg * gg
    denom = v.sqrt() / c2 + eps
    return p - (lr / c1) * (m / denom), m, v


# ---------------------------------------------------------------- occupancy step
def pseudo_grad(s_metres, g_metres, margin=2.0, free=0.25, occ=2.5):
    """oracle/occupancy.logits_pseudo_grad: +free before the surface, -occ within `margin` of it, 0 behind; steps are 0 at 0"""
    x = s_metres - g_metres
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    step = lambda t: torch.where(t > 0, one, zero)
    return free * step(-x - margin) - occ * step(x + margin) * step(margin - x)


def trilinear_scatter(V, pts, val, into=None, factor=1.0):
    """adjoint of the trilinear lookup (align_corners=False, zero padding): pts [M,3] (x,y,z), val [M] -> [V,V,V] indexed [z,y,x].
    `into`: add factor * contribution onto a copy of that grid instead of onto zeros."""
    out = (torch.zeros(V * V * V, dtype=pts.dtype) if into is None else into.reshape(-1).clone())
    idx = ((pts + 1.0) * V - 1.0) * 0.5
    base = torch.floor(idx)
    frac = idx - base
    base = base.long()
    for corner in range(8):
        off = torch.tensor([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
        c = base + off
        w3 = torch.where(off.bool(), frac, 1.0 - frac)
        w = w3[:, 0] * w3[:, 1] * w3[:, 2]
        ok = ((c >= 0) & (c < V)).all(dim=1)
        flat = (c[:, 2] * V + c[:, 1]) * V + c[:, 0]
        out.index_add_(0, flat[ok], (factor * (val * w))[ok])
    return out.reshape(V, V, V)


def occ_grad(V, rays, z, depth, scale, margin=2.0, free=0.25, occ=2.5, magnitude=False):
    """the occupancy pseudo-gradient scattered onto the grid; rays [n,13], z [n,S], depth [n].  magnitude: scatter |pseudo-gradient|
    instead - per voxel the size of what is summed there (+free and -occ meet in one voxel and cancel)"""
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
    g = pseudo_grad(z * scale, depth[:, None] * scale, margin, free, occ)
    g = g.abs() if magnitude else g
    return trilinear_scatter(V, pts.reshape(-1, 3), g.reshape(-1))


def occ_step(grid, rays, z, depth, scale, lr, margin=2.0, free=0.25, occ=2.5, in_place=False):
    """grid [V,V,V] -> grid - lr * gradient.  in_place: every contribution is added onto the grid itself, one at a time,
    as the float-atomic route does."""
    V = grid.shape[-1]
    if not in_place:
        return grid - lr * occ_grad(V, rays, z, depth, scale, margin, free, occ)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
    g = pseudo_grad(z * scale, depth[:, None] * scale, margin, free, occ)
    return trilinear_scatter(V, pts.reshape(-1, 3), g.reshape(-1), into=grid, factor=-lr)


# ---------------------------------------------------------------- input generators (float32, seeded)
COORD_AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
POSE_ANGLES = (0.0, 1e-9, 9.9e-7, 1.01e-6, 3e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 3.0,
               math.pi - 1e-3, math.pi, math.pi + 1e-3, 2 * math.pi - 1e-3, 6 * math.pi + 0.3)


def unit_axes(n, gen):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=1)


def pose_cases(seed=0):
    """-> (pose6 float32 [5 * len(POSE_ANGLES), 6], angle index [n]): per angle one random unit axis, the three coordinate axes and
    one axis with a component exactly 0; rows 5 k of consecutive angles share their axis (continuity across the series switch)"""
    gen = torch.Generator().manual_seed(seed)
    shared = unit_axes(1, gen)[0]
    rows, which = [], []
    for k, ang in enumerate(POSE_ANGLES):
        zeroed = unit_axes(1, gen)[0]
        zeroed[k % 3] = 0.0
        zeroed = zeroed / zeroed.norm()
        for ax in [shared] + [torch.tensor(a, dtype=torch.float64) for a in COORD_AXES] + [zeroed]:
            rows.append(torch.cat([torch.randn(3, generator=gen, dtype=torch.float64) * 30.0, ax * ang]))
            which.append(k)
    return torch.stack(rows).float(), torch.tensor(which)


def direction_table(n_points, gen):
    """unit directions [3, n_points] float32, isotropic"""
    return torch.nn.functional.normalize(torch.randn(3, n_points, generator=gen), dim=0).contiguous()


def segment_transform(gen, scale, shift, lo=-0.6, hi=0.6, angle=None):
    """float32 [3,4]: a rotation and a translation whose origin (t + shift) / scale is uniform in [lo, hi]^3"""
    aa = unit_axes(1, gen) * (float(torch.rand(1, generator=gen)) * 3.0 if angle is None else angle)
    R = rotation_exp(aa)[0]
    o = lo + (hi - lo) * torch.rand(3, generator=gen, dtype=torch.float64)
    t = o * scale - torch.as_tensor(shift, dtype=torch.float64)
    return torch.cat([R, t[:, None]], dim=1).float()


def log_uniform_grads(n, gen, lo=-12.0, hi=6.0):
    """float32 gradients of either sign with magnitudes log-uniform in [1e-12, 1e6]; one element in seven exactly 0"""
    mag = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g = (mag * sign).float()
    g[3::7] = 0.0
    return g


def occ_batch(V, S, n, seed, scale=85.76):
    """rays [n,13], z [n,S], depth [n] float32: origins in [-0.6, 0.6]^3 and samples up to z = 1 along unit directions, so that
    about a fifth of the samples lie outside [-1,1]^3; the surface lies at 40 % to 90 % of the ray"""
    gen = torch.Generator().manual_seed(seed)
    rays = torch.zeros(n, RAY_STRIDE)
    rays[:, 0:3] = torch.rand(n, 3, generator=gen) * 1.2 - 0.6
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=1)
    rays[:, 6:9] = -rays[:, 3:6]
    rays[:, 11], rays[:, 12] = 1.0 / scale, 1.0
    z = torch.sort(torch.rand(n, S, generator=gen), dim=1).values
    depth = 0.4 + 0.5 * torch.rand(n, generator=gen)
    return rays, z, depth


# ---------------------------------------------------------------- LiDAR window cases
LIDAR_SCALE = 85.76
LIDAR_SHIFT = (3.0, -2.0, 1.5)
LIDAR_RANGE = (1.0, 1.2 * LIDAR_SCALE)        # range_max / scale = 1.2: with origins in [-0.6, 0.6]^3 a third of the rays are range-limited
LIDAR_KEPT = (0, 1, 63, 256, 257, 1000, 0)
# seeds of the cases that tests/test_gpu_pose_tail.py runs and tests/test_tail_host.py checks the conditions of
LIDAR_SEEDS = (11, 12)
SPECIAL_SEED = 21
CHAIN_SEED = 31


def lidar_case(seed, kept=LIDAR_KEPT, special=(), poses=None):
    """A window of len(kept) segments for lnr_build_window_rays -> lnr_compact_rays -> lnr_lidar_rays_backward, all float32 / int64:
    per segment its own direction table (the sizes differ), a transform, candidate indices drawn with repeats, and a keep mask that
    drops every near-tie candidate and then more at random until exactly kept[s] rays are left.  The first segment with kept 0 has
    no candidate at all, later ones have candidates that are all dropped.  Origins are uniform in [-0.6, 0.6]^3, those of segments
    of 1000 rays or more in [-0.1, 0.1]^3, from where rays end on all six faces.
    special[s]: "zero" = identity rotation and a table whose y components are exactly 0; "outside" = origin at x in [1.2, 1.4].
    poses (float32 [n_seg, 6], optional): the transforms are transforms(poses) instead of random ones."""
    gen = torch.Generator().manual_seed(seed)
    shift = torch.tensor(LIDAR_SHIFT, dtype=torch.float64)
    far_range = LIDAR_RANGE[1] / LIDAR_SCALE
    case = dict(tables=[], T=[], idx=[], keep=[], tie=[], scale=LIDAR_SCALE, shift=LIDAR_SHIFT, ray_range=LIDAR_RANGE, kept=tuple(kept))
    seen_empty = False
    for s, k in enumerate(kept):
        kind = special[s] if s < len(special) else None
        table = direction_table(53 + 41 * s + k, gen)
        if kind == "zero":
            table[1] = 0.0
            table = torch.nn.functional.normalize(table, dim=0).contiguous()
        box = 0.1 if k >= 1000 else 0.6       # all six faces lie within range_max / scale = 1.2 only of an origin near the centre
        T = segment_transform(gen, LIDAR_SCALE, LIDAR_SHIFT, lo=-box, hi=box, angle=0.0 if kind == "zero" else None)
        if kind == "outside":
            T[0, 3] = float((1.2 + 0.2 * float(torch.rand(1, generator=gen))) * LIDAR_SCALE - LIDAR_SHIFT[0])
        if poses is not None:
            T = transforms(poses[s:s + 1].double())[0].float()
        n_cand = k + k // 3 + 5 if (k > 0 or seen_empty) else 0
        seen_empty |= k == 0
        idx = torch.randint(0, table.shape[1], (n_cand,), generator=gen)
        rec = ray_records(T.double(), table.double(), idx, LIDAR_RANGE, LIDAR_SCALE, shift)
        tie = near_tie(rec, far_range) if n_cand else torch.zeros(0, dtype=torch.bool)
        good = torch.nonzero(~tie)[:, 0]
        assert good.numel() >= k, "not enough candidates away from a tie"
        keep = torch.zeros(n_cand, dtype=torch.bool)
        keep[good[torch.randperm(good.numel(), generator=gen)[:k]]] = True
        for name, val in (("tables", table), ("T", T), ("idx", idx), ("keep", keep), ("tie", tie)):
            case[name].append(val)
    case["T"] = torch.stack(case["T"])
    return case


def lidar_records(case, T, dtype):
    """per segment the records [kept[s], 13] of the kept rays, in `dtype`, from transforms T [n_seg,3,4] (may require grad)"""
    shift = torch.tensor(case["shift"], dtype=dtype)
    return [ray_records(T[s], case["tables"][s].to(dtype), case["idx"][s][case["keep"][s]], case["ray_range"], case["scale"], shift)
            for s in range(len(case["tables"]))]


def lidar_dT(case, cot, dtype):
    """autograd of sum(cot * records) with respect to the transforms -> [n_seg,3,4]; cot: list of [kept[s],13]"""
    T = case["T"].to(dtype).requires_grad_(True)
    loss = sum((c.to(dtype) * r).sum() for c, r in zip(cot, lidar_records(case, T, dtype)))
    if not torch.is_tensor(loss) or not loss.requires_grad:
        return torch.zeros_like(T)
    return torch.autograd.grad(loss, T)[0]


# ---------------------------------------------------------------- the chain pose6 -> rays -> points -> scalar
CHAIN_ANGLES = (0.0, 2e-3, 0.7)


def chain_case(seed, rays_per_pose=300, n_samples=24):
    """three poses (|axis-angle| = 0, 2e-3, 0.7) with origins in [-0.6, 0.6]^3, each with a segment of rays_per_pose kept rays,
    fixed sample distances z in [0, 1) and weights c of the far column"""
    gen = torch.Generator().manual_seed(seed)
    n = len(CHAIN_ANGLES)
    t = (torch.rand(n, 3, generator=gen, dtype=torch.float64) * 1.2 - 0.6) * LIDAR_SCALE - torch.tensor(LIDAR_SHIFT, dtype=torch.float64)
    aa = unit_axes(n, gen) * torch.tensor(CHAIN_ANGLES, dtype=torch.float64)[:, None]
    pose6 = torch.cat([t, aa], dim=1).float()
    case = lidar_case(seed + 1, kept=(rays_per_pose,) * n, poses=pose6)
    case["pose6"] = pose6
    case["z"] = [torch.rand(rays_per_pose, n_samples, generator=gen) for _ in range(n)]
    case["c"] = [torch.randn(rays_per_pose, generator=gen) for _ in range(n)]
    return case


def chain_loss(pose6, case, form="exp"):
    """L(pose6) = sum over samples of sin(3x) + cos(2y) z + 0.5 x y at p = o + d z, plus sum(c * far); in pose6's dtype"""
    dtype = pose6.dtype
    total = 0.0
    for s, rec in enumerate(lidar_records(case, transforms(pose6, form), dtype)):
        p = rec[:, None, 0:3] + rec[:, None, 3:6] * case["z"][s].to(dtype)[..., None]
        total = total + chain_loss_terms(p) + (case["c"][s].to(dtype) * rec[:, 12]).sum()
    return total


def chain_point_grads(case):
    """what the renderer's backward would hand to the tail, formed in float64 and rounded once: d_pts [n,S,3] and the cotangent of
    far, for all kept rays of the window in order"""
    rec = torch.cat(lidar_records(case, transforms(case["pose6"].double()), torch.float64))
    z = torch.cat(case["z"]).double()
    p = (rec[:, None, 0:3] + rec[:, None, 3:6] * z[..., None]).requires_grad_(True)
    d_pts = torch.autograd.grad(chain_loss_terms(p), p)[0]
    return d_pts.float(), torch.cat(case["c"]).clone()


# ---------------------------------------------------------------- bookkeeping of the measured figures
class Ledger:
    """Collects, per named check, the worst block: every block is held to bound(), the figures are printed before anything is
    asserted, and `failures` lists the blocks that missed."""

    def __init__(self):
        self.rows, self.failures = {}, []

    def block(self, name, x, x32, x64, where=""):
        """x: the kernel's block, x32 / x64: the restatement's float32 / float64 run of the same block"""
        return self.figures(name, block_err(x, x64), block_err(x32, x64), block_max(x64), where)

    def figures(self, name, err, noise, ref_max, where=""):
        limit = 4.0 * noise + 4.0 * F32_EPS * ref_max
        ratio = err / limit if limit > 0 else (0.0 if err == 0 else float("inf"))
        norm = ref_max if ref_max > 0 else 1.0
        row = self.rows.get(name)
        if row is None or ratio >= row[0]:
            self.rows[name] = (ratio, noise / norm, err / norm, where)
        if err > limit:
            self.failures.append(f"{name} {where}: error {err:.3e} > 4 x {noise:.3e} + 4 ulp of {ref_max:.3e}")
        return err <= limit

    def report(self):
        for name, (ratio, noise, err, where) in self.rows.items():
            print(f"FIGURES {name:<44s} cpu float32 noise {noise:.2e}  kernel {err:.2e}  (of the block's largest entry; worst block {where}: {ratio:.2f} of its bound)")
        return self.failures
