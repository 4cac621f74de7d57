"""lnr_adam_step and lnr_occ_grid_step / apply against the float64 run of tests/tail_restatement.py - needs an MI355X.

Adam is compared element by element on the UPDATE (p_new - p_old) / lr and on both moments, never on p.  The error of an element is
taken relative to max(|reference|, floor); the yardstick is the same figure of the restatement's float32 run on the CPU, and the
kernel has to stay within 4 x that + 4 ulp.  Floors: the update is measured against 1 (a step of Adam is lr x O(1): this resolves
5e-7 of a step) and, on the elements whose parameter starts at 0 (no rounding of p in the way), against 1e-6; the moments against
the smallest normal float32 (exp_avg, a difference, against the larger of its two terms).  The reference receives the hyper-parameters the kernel receives: the C interface takes lr, the betas
and eps as float, so it is Adam with betas (float32(0.9), float32(0.999)) that both compute.
The occupancy step is compared per voxel in the same way (floor: what |pseudo-gradient| sums to in the voxel, and a thousandth
of the largest voxel) on the fixed-point accumulator, and as one block on the grid after the step.  "bit" is torch.equal.
The permuted-rays check caught the fixed-point route summing each run in float before converting: with n_samples = 100 the 64-sample
chunks of the flat sample list cut a ray elsewhere once the rays are reordered, and the accumulator's bits changed; the chunks are
now aligned to the ray (ceil(S/64) per ray), which leaves every S that is a multiple of 64 exactly as it was and takes
`prev_ray != ray` out of the run head, since a wave no longer straddles two rays.

Measured (CPU float32 noise | kernel on the MI355X; worst case over the parametrised shapes; last column: the kernel's error as a
fraction of its bound):

    check                                          CPU noise | kernel  of bound  (worst block)
    adam: update, against a whole step             8.7e-08 | 1.9e-07   0.23   (n = 4, step 1)
    adam: update where p starts at 0, relative     1.2e-11 | 1.9e-07   0.39   (n = 4, step 1)
    adam: exp_avg, relative                        1.5e-07 | 1.1e-07   0.10   (n = 2101155, step 100000)
    adam: exp_avg_sq, relative                     1.2e-07 | 1.2e-07   0.12   (n = 2101155, step 1)
    occ: fixed-point gradient per voxel            1.0e-05 | 1.0e-05   0.25   (V = 7, S = 64, 4 of 5 rays)
    occ: grid after grad_buf + apply               8.4e-08 | 8.4e-08   0.10   (V = 100, S = 512, 12 of 16 rays)
    occ: grid after the float-atomic step          1.3e-07 | 8.4e-08   0.08   (V = 100, S = 512, 12 of 16 rays)
"""
import math

import numpy as np
import pytest
import torch

from tests import tail_restatement as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = float(np.float32(0.01))
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
TINY = float(np.finfo(np.float32).tiny)
FIXED = 2.0 ** 42


def dv(x, dtype=torch.float32):
    return x.to(DEV, dtype).contiguous()


@pytest.fixture(scope="module")
def ops():
    from loner_amd import ops as _ops
    from loner_amd import hip
    hip.load()
    return _ops


def _finish(ledger):
    failures = ledger.report()
    assert not failures, "\n".join(failures)


def _rel(led, name, x, x32, x64, floor, where):
    """element-wise relative figures into the ledger: the bound is 4 x noise + 4 ulp of 1"""
    return led.figures(name, TR.elementwise_rel(x, x64, floor), TR.elementwise_rel(x32, x64, floor), 1.0, where)


# ------------------------------------------------------------------------------------------- a. Adam
def _adam_inputs(n, step, seed):
    """p (every other element 0), gradient, and the moments carried in: zero at step 1, else one float64 reference step (number
    step - 1) from the stationary moments of an earlier gradient, rounded to float32.  Elements 3, 10, 17, ... of every gradient are 0."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 1e-2
    p[1::2] = 0.0
    g = TR.log_uniform_grads(n, gen)
    if step == 1:
        return p, g, torch.zeros(n), torch.zeros(n)
    ga, gb = TR.log_uniform_grads(n, gen).double(), TR.log_uniform_grads(n, gen).double()
    _, m, v = TR.adam_step(p.double(), gb, ga, ga * ga, LR, step - 1, B1, B2, EPS)
    return p, g, m.float(), v.float()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 2_097_152 + 4000 + 3])
def test_adam_update_and_moments_element_by_element(ops, n):
    """the last size takes a second grid-stride trip (the grid is capped at 2048 x 256 threads x 4 floats) and the scalar tail"""
    led = TR.Ledger()
    for step in (1, 2, 1000, 100000):
        p0, g, m0, v0 = _adam_inputs(n, step, 1000 * step + n % 1000)
        p, gd, m, v = dv(p0), dv(g), dv(m0), dv(v0)
        ops.adam_step(p, gd, m, v, LR, step, betas=(B1, B2), eps=EPS)
        assert float(gd.abs().max()) == 0.0
        p, m, v = p.cpu(), m.cpu(), v.cpu()
        r32 = TR.adam_step(p0, g, m0, v0, LR, step, B1, B2, EPS)
        r64 = TR.adam_step(p0.double(), g.double(), m0.double(), v0.double(), LR, step, B1, B2, EPS)
        upd = lambda q: (q.double() - p0.double()) / LR
        where = f"n = {n}, step {step}"
        _rel(led, "adam: update, against a whole step", upd(p), upd(r32[0]), upd(r64[0]), 1.0, where)
        # exp_avg = m + (g - m) (1 - b1) cancels where g is about -9 m: its error, and that of the update it is the numerator
        # of, are taken relative to the larger of the two terms where that exceeds the result
        terms = torch.maximum(m0.abs(), g.abs() * (1.0 - B1)).double().clamp(min=TINY)
        terms_upd = (terms / (1.0 - B1 ** step) / (r64[2].sqrt() / math.sqrt(1.0 - B2 ** step) + EPS)).clamp(min=1e-6)
        at0 = p0 == 0
        _rel(led, "adam: update where p starts at 0, relative", upd(p)[at0], upd(r32[0])[at0], upd(r64[0])[at0], terms_upd[at0], where)
        _rel(led, "adam: exp_avg, relative", m, r32[1], r64[1], terms, where)
        _rel(led, "adam: exp_avg_sq, relative", v, r32[2], r64[2], TINY, where)
        # a zero gradient on zero moments: the parameter keeps its bits
        assert torch.equal(p[3::7], p0[3::7]) and not bool(m[3::7].any()) and not bool(v[3::7].any())
    _finish(led)


def _state(n, seed, step=3):
    p0, g, m0, v0 = _adam_inputs(n, step, seed)
    return [dv(p0), dv(g), dv(m0), dv(v0)]


def test_adam_grad_scale_and_zero_grad(ops):
    n = 10003
    a, b = _state(n, 5), _state(n, 5)
    b[1] = b[1] / 128.0                                      # exact: a power of two, no gradient near the subnormals
    g_before = a[1].clone()
    ops.adam_step(*a, LR, 3, betas=(B1, B2), eps=EPS, grad_scale=1.0 / 128.0, zero_grad=False)
    ops.adam_step(*b, LR, 3, betas=(B1, B2), eps=EPS, zero_grad=True)
    for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
        assert torch.equal(x, y)
    assert torch.equal(a[1], g_before)                       # zero_grad=False leaves the gradient's bits alone
    assert float(b[1].abs().max()) == 0.0                    # zero_grad=True clears all of it, tail included
    assert not torch.equal(a[0], _state(n, 5)[0])


def test_adam_on_views_of_one_buffer(ops):
    n, lo, hi = 10003, 2048, 7300                            # lo and hi are multiples of 4: every piece is 16-byte aligned
    whole, pieces, single = _state(n, 6), _state(n, 6), _state(n, 6)
    before = [t.clone() for t in single]
    ops.adam_step(*whole, LR, 3, betas=(B1, B2), eps=EPS)
    for a, b in ((0, lo), (lo, hi), (hi, n)):
        ops.adam_step(*[t[a:b] for t in pieces], LR, 3, betas=(B1, B2), eps=EPS)
    for x, y in zip(whole, pieces):
        assert torch.equal(x, y)
    # one piece: everything outside it keeps its bits - parameters, gradient and both moments
    ops.adam_step(*[t[lo:hi] for t in single], LR, 3, betas=(B1, B2), eps=EPS)
    for x, y, w in zip(single, before, whole):
        assert torch.equal(x[:lo], y[:lo]) and torch.equal(x[hi:], y[hi:]) and torch.equal(x[lo:hi], w[lo:hi])
    # a view that starts at an odd element is refused, and nothing has moved
    odd = _state(n, 6)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.adam_step(*[t[1:] for t in odd], LR, 3, betas=(B1, B2), eps=EPS)
    for x, y in zip(odd, before):
        assert torch.equal(x, y)


def test_hip_adam_ranges_equal_one_whole_step(ops):
    from loner_amd.mapping.optimizer import HipAdam
    n, lo, hi = 10003, 2048, 7300
    results = []
    for ranges in (None, [(0, lo), (lo, hi), (hi, n)]):
        p0, g, _, _ = _adam_inputs(n, 1, 9)
        param = torch.nn.Parameter(dv(p0))
        opt = HipAdam([dict(params=[param], lr=LR)])
        for k in range(3):
            param.grad = dv(g) * (0.5 ** k)
            opt.step(zero_grad=True, ranges=ranges)
            assert float(param.grad.abs().max()) == 0.0
        st = opt.state[param]
        assert st["step"] == 3
        results.append((param.data.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    for x, y in zip(*results):
        assert torch.equal(x, y)
    # a single range: the rest of the parameter and of its moments does not move
    p0, g, _, _ = _adam_inputs(n, 1, 9)
    param = torch.nn.Parameter(dv(p0))
    opt = HipAdam([dict(params=[param], lr=LR)])
    param.grad = dv(g)
    opt.step(zero_grad=False, ranges=[(lo, hi)])
    st = opt.state[param]
    for x, y in ((param.data, dv(p0)), (st["exp_avg"], torch.zeros(n, device=DEV)), (st["exp_avg_sq"], torch.zeros(n, device=DEV)), (param.grad, dv(g))):
        assert torch.equal(x[:lo], y[:lo]) and torch.equal(x[hi:], y[hi:])
    assert not torch.equal(param.data[lo:hi], dv(p0)[lo:hi])


# ------------------------------------------------------------------------------------------- b. occupancy step
SCALE, OCC_LR = float(np.float32(85.76)), 1e-2                # the kernel receives its scale as a float


def _occ_case(V, S, n, seed=5):
    rays, z, depth = TR.occ_batch(V, S, n, seed)
    live = n - max(1, n // 4)
    grid0 = torch.randn(V, V, V, generator=torch.Generator().manual_seed(seed + 1))
    return rays, z, depth, live, grid0


def _fixed_point_step(ops, grid0, rays, z, depth, live, lr=OCC_LR, scale=SCALE):
    V = grid0.shape[-1]
    grid = dv(grid0)
    buf = torch.zeros(V ** 3, device=DEV, dtype=torch.int64)
    count = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
    ops.occ_grid_step(grid, dv(rays), dv(z), dv(depth), scale, lr, grad_buf=buf, n_rays_dev=count)
    assert torch.equal(grid.cpu(), grid0)                     # the first stage only accumulates
    acc = buf.cpu().clone()
    ops.occ_grid_apply(grid, buf, lr)
    assert int(buf.abs().max()) == 0                          # apply re-zeroes what it applied
    return grid.cpu(), acc


@pytest.mark.parametrize("V,S,n", [(24, 100, 37), (100, 512, 16), (7, 64, 5)])
def test_occ_grid_step_per_voxel(ops, V, S, n):
    """S = 100: a ray is no whole number of 64-sample chunks; the rows from `live` on hold samples that would change the grid if they were read"""
    rays, z, depth, live, grid0 = _occ_case(V, S, n)
    where = f"V = {V}, S = {S}, {live} of {n} rays"
    lr32 = float(np.float32(OCC_LR))
    args64 = (rays[:live].double(), z[:live].double(), depth[:live].double(), SCALE)
    grad64 = TR.occ_grad(V, *args64)
    grad32 = TR.occ_grad(V, rays[:live], z[:live], depth[:live], SCALE)
    dead = TR.occ_grad(V, rays[live:].double(), z[live:].double(), depth[live:].double(), SCALE)
    assert float(dead.abs().max()) > 0
    led = TR.Ledger()
    # fixed-point route
    grid, acc = _fixed_point_step(ops, grid0, rays, z, depth, live)
    floor = TR.occ_grad(V, *args64, magnitude=True).clamp(min=1e-3 * float(grad64.abs().max()))
    _rel(led, "occ: fixed-point gradient per voxel", acc.double().reshape(V, V, V) / FIXED, grad32, grad64, floor, where)
    led.block("occ: grid after grad_buf + apply", grid, TR.occ_step(grid0, rays[:live], z[:live], depth[:live], SCALE, lr32),
              TR.occ_step(grid0.double(), *args64, lr32), where)
    # the set of changed voxels is the reference's, but for voxels whose update is below 2^-40
    changed, expected = (acc != 0).reshape(V, V, V), grad64 != 0
    assert not bool((changed & ~expected).any())
    missed = expected & ~changed
    assert float((lr32 * grad64[missed]).abs().max() if bool(missed.any()) else 0.0) < 2.0 ** -40, int(missed.sum())
    # the same rays in another order: the same bits
    perm = torch.cat([torch.randperm(live, generator=torch.Generator().manual_seed(3)), torch.arange(live, n)])
    grid_p, acc_p = _fixed_point_step(ops, grid0, rays[perm], z[perm], depth[perm], live)
    assert torch.equal(acc_p, acc) and torch.equal(grid_p, grid)
    # float-atomic route: every contribution lands on the grid itself
    grid_f = dv(grid0)
    ops.occ_grid_step(grid_f, dv(rays), dv(z), dv(depth), SCALE, OCC_LR, n_rays_dev=torch.tensor([live], dtype=torch.int32, device=DEV))
    led.block("occ: grid after the float-atomic step", grid_f.cpu(), TR.occ_step(grid0, rays[:live], z[:live], depth[:live], SCALE, lr32, in_place=True),
              TR.occ_step(grid0.double(), *args64, lr32), where)
    assert torch.equal(grid_f.cpu()[~expected], grid0[~expected])
    _finish(led)


def test_occ_grid_step_known_answers(ops):
    """scale 1, depth 4, margin 2, V = 8, lr = 2^-7, directions 0 so that every sample of a ray sits on the ray's origin, a voxel
    centre: x = -margin and x = +margin contribute nothing, the next float32 x on either side of -margin and below +margin
    contributes -occ / +free / -occ with weight 1"""
    V, S, lr = 8, 5, 2.0 ** -7
    centre = lambda i: (2 * i + 1) / V - 1.0
    vox = [(2, 5, 7), (1, 1, 1), (6, 0, 3), (4, 4, 0), (0, 7, 5), (3, 2, 6)]                 # (x, y, z) voxel of each ray
    # x = z - 4 is exact for each of these: -2, +2, 0, and the float32 neighbours of -2 (either side) and of +2 (below)
    zs = [2.0, 6.0, 4.0, 2.0 + 2.0 ** -22, 2.0 - 2.0 ** -22, 6.0 - 2.0 ** -21]
    gval = [0.0, 0.0, -2.5, -2.5, 0.25, -2.5]
    rays = torch.zeros(len(vox), 13)
    rays[:, 0:3] = torch.tensor([[centre(i) for i in v] for v in vox])
    z = torch.tensor(zs)[:, None].expand(len(vox), S).contiguous()
    depth = torch.full((len(vox),), 4.0)
    expect = torch.zeros(V, V, V)
    for (x, y, zz), g in zip(vox, gval):
        expect[zz, y, x] = -(torch.tensor(lr) * torch.tensor(S * g))
    assert int((expect != 0).sum()) == 4
    grid, acc = _fixed_point_step(ops, torch.zeros(V, V, V), rays, z, depth, None, lr=lr, scale=1.0)
    assert torch.equal(grid, expect)
    assert torch.equal(acc.reshape(V, V, V), (expect.double() / -lr * FIXED).long())
    grid_f = torch.zeros(V, V, V, device=DEV)
    ops.occ_grid_step(grid_f, dv(rays), dv(z), dv(depth), 1.0, lr)
    assert torch.equal(grid_f.cpu(), expect)
    assert float((TR.occ_step(torch.zeros(V, V, V, dtype=torch.float64), rays.double(), z.double(), depth.double(), 1.0, lr) - expect.double()).abs().max()) == 0.0


def test_occ_grid_step_behind_the_surface_changes_nothing(ops):
    V, S, n = 24, 100, 37
    rays, z, depth, _, grid0 = _occ_case(V, S, n)
    z = depth[:, None] + 2.5 / SCALE + 0.3 * torch.rand(n, S, generator=torch.Generator().manual_seed(1))
    assert float(TR.occ_grad(V, rays.double(), z.double(), depth.double(), SCALE).abs().max()) == 0.0
    grid, acc = _fixed_point_step(ops, grid0, rays, z, depth, None)
    assert torch.equal(grid, grid0) and int(acc.abs().max()) == 0
    grid_f = dv(grid0)
    ops.occ_grid_step(grid_f, dv(rays), dv(z), dv(depth), SCALE, OCC_LR)
    assert torch.equal(grid_f.cpu(), grid0)


def test_occ_grid_step_refuses_grids_its_run_key_cannot_hold(ops):
    rays, z, depth = TR.occ_batch(8, 4, 2, seed=1)
    grid = torch.zeros(1, 1024, device=DEV)                   # only the last dimension is read as V before the refusal
    with pytest.raises(RuntimeError, match="1023"):
        ops.occ_grid_step(grid, dv(rays), dv(z), dv(depth), SCALE, OCC_LR)
    assert float(grid.abs().max()) == 0.0
