"""The kernels that turn d_rays into a pose gradient, against float64 autograd of tests/tail_restatement.py - needs an MI355X.

Every floating-point check is made PER BLOCK against that block's own largest reference entry: the rotation 3x3 and the translation
column of each segment's dT, the translation rows and the axis-angle rows of each pose's gradient, the columns 0:3, 3:6 and 12 of
d_rays.  A block passes when its error is at most 4 x (the error of the restatement's float32 run on the CPU, same inputs, same
block) + 4 ulp of the block's largest reference entry; nothing is derived from the kernel's output.  "bit" is torch.equal.

Measured (CPU float32 noise | kernel on the MI355X, both relative to the block's largest entry, at the block that came closest
to its bound; last column: that block's error as a fraction of its bound):

    check                                          CPU noise | kernel  of bound  (worst block)
    pose_forward R                                 9.2e-07 | 9.2e-07   0.22   (pose 165 angle 19.1)
    pose_forward R^T R - I                         1.4e-07 | 2.9e-07   0.27   (pose 149 angle 3.14)
    pose_backward axis-angle rows                  2.3e-08 | 2.5e-07   0.44   (pose 147 angle 3.14)
    pose_backward accumulate                       1.8e-07 | 3.5e-07   0.30   (pose 10)
    series switch: R(1.01e-6) - R(9.9e-7)          2.0e-14 | 2.0e-14   0.00   ()
    series switch: gradient step                   2.2e-08 | 2.2e-08   0.04   ()
    7 segments: records, origin                    7.0e-08 | 7.0e-08   0.09   (segment 3)
    7 segments: records, direction                 8.1e-08 | 9.5e-08   0.12   (segment 4)
    7 segments: records, far                       1.6e-07 | 1.6e-07   0.14   (segment 5)
    7 segments: dT rotation 3x3                    9.8e-08 | 1.2e-07   0.13   (segment 1 (1 rays))
    7 segments: dT translation column              5.1e-07 | 4.6e-07   0.18   (segment 3 (256 rays))
    special segments: records, origin              3.5e-08 | 3.5e-08   0.06   (segment 0)
    special segments: records, direction           9.3e-08 | 9.3e-08   0.11   (segment 1)
    special segments: records, far                 8.9e-08 | 8.4e-08   0.10   (segment 1)
    special segments: dT rotation 3x3              6.3e-07 | 4.3e-07   0.14   (segment 0 (200 rays))
    special segments: dT translation column        2.6e-07 | 5.0e-08   0.03   (segment 0 (200 rays))
    points_grad_to_rays: origin columns            1.2e-07 | 1.3e-07   0.14   (S = 512)
    points_grad_to_rays: direction columns         9.3e-08 | 1.0e-07   0.12   (S = 64, all rows)
    chain: translation rows                        1.5e-07 | 7.5e-08   0.07   (pose 0 angle 0)
    chain: axis-angle rows                         1.6e-07 | 2.7e-07   0.24   (pose 1 angle 0.002)

Not every slip can show in float32: below the 1e-6 rad switch the d(sin(h)/theta)/d(theta) term of pose_backward contributes
theta^2 / 24 <= 4e-14 of the gradient, so its sign is beyond any float32 comparison (tried: all of these tests pass with it flipped).
"""
import pytest
import torch

from tests import tail_restatement as TR
from tests.tail_restatement import CHAIN_SEED, LIDAR_SEEDS, SPECIAL_SEED

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64


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


# ------------------------------------------------------------------------------------------- a. pose forward / backward
def _pose_batch(n):
    cases, which = TR.pose_cases(0)
    rows = torch.arange(n) % cases.shape[0]
    return cases[rows].clone(), which[rows]


def _pose_grads(p, cot):
    """(float32 quaternion-form autograd, float64 exponential-map autograd) of sum(cot * [R|t])"""
    pr = p.clone().requires_grad_(True)
    g32 = torch.autograd.grad((TR.transforms(pr, "quat") * cot.reshape(-1, 3, 4)).sum(), pr)[0]
    pd = p.double().requires_grad_(True)
    g64 = torch.autograd.grad((TR.transforms(pd, "exp") * cot.double().reshape(-1, 3, 4)).sum(), pd)[0]
    return g32, g64


@pytest.mark.parametrize("n", [0, 1, 64, 65, 200])
def test_pose_forward_against_the_exponential_map(ops, n):
    p, which = _pose_batch(n)
    T = ops.pose_forward(dv(p).reshape(n, 6))
    assert T.shape == (n, 12)
    T = T.cpu().reshape(n, 3, 4)
    ours, truth = TR.transforms(p, "quat"), TR.transforms(p.double(), "exp")
    assert torch.equal(T[:, :, 3], p[:, 0:3])                                     # the translation is copied
    eye = torch.eye(3, dtype=F64)
    led = TR.Ledger()
    for i in range(n):
        where = f"pose {i} angle {TR.POSE_ANGLES[int(which[i])]:.3g}"
        led.block("pose_forward R", T[i, :, :3], ours[i, :, :3], truth[i, :, :3], where)
        defect = lambda R: R.double().T @ R.double() - eye
        led.figures("pose_forward R^T R - I", float(defect(T[i, :, :3]).abs().max()), float(defect(ours[i, :, :3]).abs().max()), 1.0, where)
    _finish(led)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 200])
def test_pose_backward_per_pose_and_per_block(ops, n):
    p, which = _pose_batch(n)
    gen = torch.Generator().manual_seed(100 + n)
    cot = torch.randn(n, 12, generator=gen)
    g32, g64 = _pose_grads(p, cot)
    pd, cd = dv(p).reshape(n, 6), dv(cot).reshape(n, 12)
    g = ops.pose_backward(pd, cd)
    assert g.shape == (n, 6)
    g = g.cpu()
    assert torch.equal(g[:, 0:3], cot[:, [3, 7, 11]])                             # mask=None: the translation gradient is G[3], G[7], G[11]
    led = TR.Ledger()
    for i in range(n):
        led.block("pose_backward axis-angle rows", g[i, 3:6], g32[i, 3:6], g64[i, 3:6], f"pose {i} angle {TR.POSE_ANGLES[int(which[i])]:.3g}")
    # an all-zero mask: every gradient exactly 0
    zero = ops.pose_backward(pd, cd, mask=torch.zeros(n, dtype=torch.uint8, device=DEV))
    assert torch.equal(zero.cpu(), torch.zeros(n, 6))
    # accumulate=True onto a non-zero `out`: a masked row keeps its bits, the others receive previous + gradient
    mask = (torch.rand(n, generator=gen) < 0.7).to(torch.uint8)
    prev = torch.randn(n, 6, generator=gen)
    out = ops.pose_backward(pd, cd, mask=mask.to(DEV), out=dv(prev).reshape(n, 6), accumulate=True).cpu()
    off = mask == 0
    assert torch.equal(out[off], prev[off])
    on = torch.nonzero(mask)[:, 0].tolist()
    for i in on:
        assert torch.equal(out[i, 0:3], prev[i, 0:3] + cot[i, [3, 7, 11]])
        led.block("pose_backward accumulate", out[i, 3:6], prev[i, 3:6] + g32[i, 3:6], prev[i, 3:6].double() + g64[i, 3:6], f"pose {i}")
    # accumulate=False with a mask: masked rows are exactly 0, `out` is overwritten
    out = ops.pose_backward(pd, cd, mask=mask.to(DEV), out=dv(prev).reshape(n, 6), accumulate=False).cpu()
    assert torch.equal(out[off], torch.zeros(int(off.sum()), 6)) and torch.equal(out[~off], g[~off])
    _finish(led)


def test_pose_kernels_are_continuous_across_the_series_switch(ops):
    """9.9e-7 and 1.01e-6 rad about the same axis, the same cotangent: R and the gradient move by what the exponential map moves"""
    cases, which = TR.pose_cases(0)
    a, b = 5 * TR.POSE_ANGLES.index(9.9e-7), 5 * TR.POSE_ANGLES.index(1.01e-6)
    p = cases[[a, b]].clone()
    p[1, 0:3] = p[0, 0:3]
    axis = lambda v: v[3:6].double() / v[3:6].double().norm()
    assert float((axis(p[0]) - axis(p[1])).abs().max()) < 1e-6
    cot = torch.randn(1, 12, generator=torch.Generator().manual_seed(7)).expand(2, 12).contiguous()
    g32, g64 = _pose_grads(p, cot)
    T = ops.pose_forward(dv(p)).cpu().reshape(2, 3, 4)
    g = ops.pose_backward(dv(p), dv(cot)).cpu()
    ours, truth = TR.transforms(p, "quat"), TR.transforms(p.double(), "exp")
    led = TR.Ledger()
    step = lambda x: x[1].double() - x[0].double()
    led.figures("series switch: R(1.01e-6) - R(9.9e-7)", TR.block_err(step(T[:, :, :3]), step(truth[:, :, :3])),
                TR.block_err(step(ours[:, :, :3]), step(truth[:, :, :3])), TR.block_max(truth[0, :, :3]))
    led.figures("series switch: gradient step", TR.block_err(step(g[:, 3:6]), step(g64[:, 3:6])),
                TR.block_err(step(g32[:, 3:6]), step(g64[:, 3:6])), TR.block_max(g64[0, 3:6]))
    _finish(led)


# ------------------------------------------------------------------------------------------- b. lidar_rays_backward
def _window(ops, case, transforms12=None, seg_pose=None):
    """build_window_rays on the case's candidates, compact_rays with the case's keep mask -> what the training loop holds"""
    n_seg = len(case["tables"])
    tables = [dv(t) for t in case["tables"]]
    counts = [len(i) for i in case["idx"]]
    tab = ops.WindowTables(tables, [None] * n_seg, [1.0] * n_seg, counts, seg_pose if seg_pose is not None else list(range(n_seg)))
    T12 = dv(case["T"].reshape(n_seg, 12)) if transforms12 is None else transforms12
    idx = torch.cat(case["idx"]).to(DEV)
    keep = torch.cat(case["keep"]).to(torch.uint8).to(DEV)
    rays, depths, _, src = ops.build_window_rays(tab, T12, case["ray_range"], case["scale"], case["shift"], index=idx)
    rays_c, _, src_c, seg_dev, n_out = ops.compact_rays(rays, depths, keep, src, tab.seg_start_list)
    starts = [0]
    for k in case["kept"]:
        starts.append(starts[-1] + k)
    assert seg_dev.cpu().tolist() == starts and int(n_out) == starts[-1]
    assert torch.equal(src_c[:starts[-1]].cpu(), torch.cat([i[k] for i, k in zip(case["idx"], case["keep"])]))
    return dict(tables=tables, T12=T12, rays=rays_c, src=src_c, seg_dev=seg_dev, n_out=n_out, starts=starts)


def _check_records(led, case, win, name):
    """the compacted records against the float64 restatement, per segment and column block"""
    r32 = TR.lidar_records(case, case["T"], F32)
    r64 = TR.lidar_records(case, case["T"].double(), F64)
    rays = win["rays"].cpu()
    for s, k in enumerate(case["kept"]):
        got = rays[win["starts"][s]:win["starts"][s + 1]]
        if k == 0:
            continue
        for cols, what in ((slice(0, 3), "origin"), (slice(3, 6), "direction"), (slice(12, 13), "far")):
            led.block(f"{name}: records, {what}", got[:, cols], r32[s][:, cols], r64[s][:, cols], f"segment {s}")
        assert torch.equal(got[:, 6:9], -got[:, 3:6]) and float(got[:, 9:11].abs().max()) == 0.0


def _check_dT(led, case, win, dT, cot, name):
    g32, g64 = TR.lidar_dT(case, cot, F32), TR.lidar_dT(case, cot, F64)
    dT = dT.cpu().reshape(-1, 3, 4)
    for s, k in enumerate(case["kept"]):
        if k == 0:
            assert torch.equal(dT[s], torch.zeros(3, 4)), f"segment {s} has no ray: its gradient is exactly 0"
            continue
        led.block(f"{name}: dT rotation 3x3", dT[s, :, :3], g32[s, :, :3], g64[s, :, :3], f"segment {s} ({k} rays)")
        led.block(f"{name}: dT translation column", dT[s, :, 3], g32[s, :, 3], g64[s, :, 3], f"segment {s} ({k} rays)")


def _cotangent(case, win, seed):
    """random in all 13 columns for the live rows; the rows behind them hold values that would show if they were read"""
    gen = torch.Generator().manual_seed(seed)
    cot = [torch.randn(k, 13, generator=gen) for k in case["kept"]]
    d_rays = torch.full((win["rays"].shape[0], 13), 1e6)
    d_rays[:win["starts"][-1]] = torch.cat(cot)
    return cot, dv(d_rays)


@pytest.mark.parametrize("seed", LIDAR_SEEDS)
def test_lidar_rays_backward_seven_segments_after_compaction(ops, seed):
    case = TR.lidar_case(seed)
    win = _window(ops, case)
    cot, d_rays = _cotangent(case, win, seed + 1000)
    dT = ops.lidar_rays_backward(d_rays, win["rays"], win["src"], win["seg_dev"], win["tables"], win["T12"], case["scale"])
    led = TR.Ledger()
    _check_records(led, case, win, "7 segments")
    _check_dT(led, case, win, dT, cot, "7 segments")
    _finish(led)


def test_lidar_rays_backward_zero_direction_component_and_origin_outside_the_cube(ops):
    case = TR.lidar_case(SPECIAL_SEED, kept=(200, 200), special=("zero", "outside"))
    win = _window(ops, case)
    rays = win["rays"].cpu()
    assert float(rays[:200, 4].abs().max()) == 0.0                               # segment 0: d_y exactly 0
    out = rays[200:400, 3] > 0
    assert int(out.sum()) >= 20 and float(rays[200:400][out, 12].abs().max()) == 0.0   # segment 1: t_raw <= 0, far = 0
    cot, d_rays = _cotangent(case, win, 77)
    dT = ops.lidar_rays_backward(d_rays, win["rays"], win["src"], win["seg_dev"], win["tables"], win["T12"], case["scale"])
    led = TR.Ledger()
    _check_records(led, case, win, "special segments")
    _check_dT(led, case, win, dT, cot, "special segments")
    # the rays with far = 0 alone: their far cotangent reaches nothing
    only = [torch.zeros_like(cot[0]), torch.zeros_like(cot[1])]
    only[1][out, 12] = cot[1][out, 12]
    d_only = torch.zeros_like(d_rays)
    d_only[200:400] = dv(only[1])
    dT0 = ops.lidar_rays_backward(d_only, win["rays"], win["src"], win["seg_dev"], win["tables"], win["T12"], case["scale"])
    assert torch.equal(dT0.cpu(), torch.zeros(2, 12))
    _finish(led)


# ------------------------------------------------------------------------------------------- c. points_grad_to_rays
@pytest.mark.parametrize("S", [1, 63, 64, 65, 100, 512])
def test_points_grad_to_rays_accumulates_into_the_live_rows(ops, S):
    n, live = 37, 20
    gen = torch.Generator().manual_seed(S)
    d_pts = torch.randn(n, S, 3, generator=gen)
    z = torch.rand(n, S, generator=gen) * 1.5
    prev = torch.randn(n, 13, generator=gen)
    d_rays = dv(prev)
    ops.points_grad_to_rays(dv(d_pts), dv(z), d_rays, n_rays_dev=torch.tensor([live], dtype=torch.int32, device=DEV))
    got = d_rays.cpu()
    assert torch.equal(got[:, 6:], prev[:, 6:]) and torch.equal(got[live:], prev[live:])
    r32 = prev[:, 0:6] + TR.points_grad_to_rays(d_pts, z)
    r64 = prev[:, 0:6].double() + TR.points_grad_to_rays(d_pts.double(), z.double())
    led = TR.Ledger()
    for cols, what in ((slice(0, 3), "origin"), (slice(3, 6), "direction")):
        led.block(f"points_grad_to_rays: {what} columns", got[:live, cols], r32[:live, cols], r64[:live, cols], f"S = {S}")
    # without a device count every row is live
    d_all = dv(prev)
    ops.points_grad_to_rays(dv(d_pts), dv(z), d_all)
    assert torch.equal(d_all.cpu()[:live], got[:live]) and torch.equal(d_all.cpu()[:, 6:], prev[:, 6:])
    for cols, what in ((slice(0, 3), "origin"), (slice(3, 6), "direction")):
        led.block(f"points_grad_to_rays: {what} columns", d_all.cpu()[:, cols], r32[:, cols], r64[:, cols], f"S = {S}, all rows")
    _finish(led)


# ------------------------------------------------------------------------------------------- d. the chain
def test_chain_from_point_gradients_to_the_pose_gradient(ops):
    """L = sum over samples of sin(3x) + cos(2y) z + 0.5 x y at p = o + d z, plus sum(c far): d_pts and the far cotangent are formed
    in float64 and rounded once, then points_grad_to_rays -> lidar_rays_backward -> pose_backward against float64 autograd of
    L(pose6)"""
    case = TR.chain_case(CHAIN_SEED)
    n = len(TR.CHAIN_ANGLES)
    pose6 = dv(case["pose6"])
    T12 = ops.pose_forward(pose6)
    assert torch.equal(T12.cpu().reshape(n, 3, 4)[:, :, 3], case["pose6"][:, 0:3])
    win = _window(ops, case, transforms12=T12)
    live = win["starts"][-1]
    d_pts, c = TR.chain_point_grads(case)
    z = torch.cat(case["z"])
    d_rays = torch.zeros(win["rays"].shape[0], 13)
    d_rays[:live, 12] = c
    d_rays = dv(d_rays)
    ops.points_grad_to_rays(dv(d_pts), dv(z), d_rays, n_rays_dev=win["n_out"])
    dT = ops.lidar_rays_backward(d_rays, win["rays"], win["src"], win["seg_dev"], win["tables"], T12, case["scale"])
    g = ops.pose_backward(pose6, dT).cpu()
    p32 = case["pose6"].clone().requires_grad_(True)
    g32 = torch.autograd.grad(TR.chain_loss(p32, case, "quat"), p32)[0]
    p64 = case["pose6"].double().requires_grad_(True)
    g64 = torch.autograd.grad(TR.chain_loss(p64, case, "exp"), p64)[0]
    led = TR.Ledger()
    for i in range(n):
        led.block("chain: translation rows", g[i, 0:3], g32[i, 0:3], g64[i, 0:3], f"pose {i} angle {TR.CHAIN_ANGLES[i]:g}")
        led.block("chain: axis-angle rows", g[i, 3:6], g32[i, 3:6], g64[i, 3:6], f"pose {i} angle {TR.CHAIN_ANGLES[i]:g}")
    _finish(led)
