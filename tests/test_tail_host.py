"""tests/tail_restatement.py checked without a GPU: its float64 autograd against central finite differences, its float32 run against
the pinned oracle functions (the oracle is held to the bound a kernel is held to: 4 x float32 noise + 4 ulp of the block), and the
conditions that its input generators promise to the GPU tests."""
import math

import pytest
import torch

from oracle import mapping_step as MS
from oracle import occupancy as OC
from oracle import poses as OP
from oracle import rays as OR
from tests import tail_restatement as TR

LIDAR_SEEDS, SPECIAL_SEED, CHAIN_SEED = TR.LIDAR_SEEDS, TR.SPECIAL_SEED, TR.CHAIN_SEED       # the cases the GPU tests run


def _within(x, x32, x64):
    """x (the oracle's float32 result) is as close to the float64 truth as a kernel has to be"""
    return TR.block_err(x, x64) <= TR.bound(TR.block_err(x32, x64), x64)


# ------------------------------------------------------------------------------------------- the reference proves itself
def test_autograd_of_the_chain_agrees_with_central_differences():
    case = TR.chain_case(CHAIN_SEED, rays_per_pose=60, n_samples=6)
    p0 = case["pose6"].double()
    p = p0.clone().requires_grad_(True)
    grad = torch.autograd.grad(TR.chain_loss(p, case), p)[0]
    fd = torch.zeros_like(p0)
    for i in range(p0.shape[0]):
        for j in range(6):
            h = 1e-3 if j < 3 else 1e-6            # translations are metres: 1e-3 m is 1.2e-5 of the cube
            e = torch.zeros_like(p0)
            e[i, j] = h
            fd[i, j] = (TR.chain_loss(p0 + e, case) - TR.chain_loss(p0 - e, case)) / (2 * h)
    for i in range(p0.shape[0]):
        for blk in (slice(0, 3), slice(3, 6)):
            assert TR.block_err(fd[i, blk], grad[i, blk]) <= 1e-7 * TR.block_max(grad[i, blk]), (i, blk, fd[i], grad[i])


def test_exponential_map_and_quaternion_form_agree_in_float64():
    p, _ = TR.pose_cases(0)
    a, b = TR.rotation_exp(p[:, 3:6].double()), TR.rotation_quat(p[:, 3:6].double())
    assert TR.block_err(a, b) < 1e-13 * (1 + 6 * math.pi)          # the angle's own rounding grows with the angle
    eye = torch.eye(3, dtype=torch.float64)
    assert TR.block_err(a.transpose(1, 2) @ a, eye.expand_as(a)) < 1e-13


# ------------------------------------------------------------------------------------------- float32 run against the oracle
def test_float32_pose_restatement_is_the_oracle():
    p, _ = TR.pose_cases(0)
    ours = TR.transforms(p, "quat")
    theirs = torch.stack([OP.transform_from_pose6(row)[:3, :4] for row in p])
    truth = TR.transforms(p.double(), "exp")
    for i in range(p.shape[0]):
        assert _within(theirs[i, :, :3], ours[i, :, :3], truth[i, :, :3]), i
        assert torch.equal(theirs[i, :, 3], p[i, 0:3])
    # and its autograd
    po = p.clone().requires_grad_(True)
    cot = torch.randn(p.shape[0], 3, 4, generator=torch.Generator().manual_seed(1))
    torch.stack([OP.transform_from_pose6(row)[:3, :4] for row in po]).backward(cot)
    pr = p.clone().requires_grad_(True)
    g32 = torch.autograd.grad((TR.transforms(pr, "quat") * cot).sum(), pr)[0]
    pd = p.double().requires_grad_(True)
    g64 = torch.autograd.grad((TR.transforms(pd, "exp") * cot.double()).sum(), pd)[0]
    for i in range(p.shape[0]):
        assert _within(po.grad[i, 3:6], g32[i, 3:6], g64[i, 3:6]), (i, po.grad[i], g64[i])
        assert torch.equal(po.grad[i, 0:3], cot[i, :, 3])


def test_float32_ray_records_agree_with_the_oracle():
    case = TR.lidar_case(LIDAR_SEEDS[0])
    shift = torch.tensor(case["shift"])
    for s in range(len(case["kept"])):
        idx = case["idx"][s][case["keep"][s]]
        if idx.numel() == 0:
            continue
        T4 = torch.cat([case["T"][s], torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
        theirs, _, keep = OR.lidar_ray_records(case["tables"][s], torch.ones(case["tables"][s].shape[1]), idx, T4,
                                               case["ray_range"], case["scale"], shift, keep_all=True)
        assert bool(keep.all())
        ours = TR.ray_records(case["T"][s], case["tables"][s], idx, case["ray_range"], case["scale"], shift)
        truth = TR.ray_records(case["T"][s].double(), case["tables"][s].double(), idx, case["ray_range"], case["scale"], shift.double())
        for cols in (slice(0, 3), slice(3, 6), slice(6, 9), slice(11, 12), slice(12, 13)):
            assert _within(theirs[:, cols], ours[:, cols], truth[:, cols]), (s, cols)
        assert float(theirs[:, 9:11].abs().max()) == 0.0 and float(ours[:, 9:11].abs().max()) == 0.0


def test_float32_adam_restatement_agrees_with_the_oracle():
    gen = torch.Generator().manual_seed(3)
    n = 4001
    p0 = torch.randn(n, generator=gen) * 1e-2
    p_o = p0.clone()
    adam = MS.AdamState([p_o], [0.01])
    s32 = (p0.clone(), torch.zeros(n), torch.zeros(n))
    s64 = (p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
    for step in range(1, 4):
        g = TR.log_uniform_grads(n, gen)
        adam.step([g])
        s32 = TR.adam_step(s32[0], g, s32[1], s32[2], 0.01, step)
        s64 = TR.adam_step(s64[0], g.double(), s64[1], s64[2], 0.01, step)
        floor_p = 1e-2
        for theirs, a, b, floor in ((p_o, s32[0], s64[0], floor_p), (adam.m[0], s32[1], s64[1], 1e-30), (adam.v[0], s32[2], s64[2], 1e-30)):
            assert TR.elementwise_rel(theirs, b, floor) <= 4 * TR.elementwise_rel(a, b, floor) + 4 * TR.F32_EPS
    assert torch.equal(p_o[3::7], p0[3::7])          # zero gradient, zero moments: the parameter does not move


@pytest.mark.parametrize("V,S,n", [(24, 100, 37), (7, 64, 5)])
def test_float32_occupancy_step_agrees_with_the_oracle(V, S, n):
    rays, z, depth = TR.occ_batch(V, S, n, seed=5)
    scale, lr = 85.76, 1e-2
    grid0 = torch.randn(V, V, V, generator=torch.Generator().manual_seed(6))
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
    theirs = OC.grid_step(grid0[None, None], pts, z * scale, depth[:, None] * scale, lr)[0, 0]
    ours = TR.occ_step(grid0, rays, z, depth, scale, lr)
    truth = TR.occ_step(grid0.double(), rays.double(), z.double(), depth.double(), scale, lr)
    assert float((truth - grid0.double()).abs().max()) > 0
    assert _within(theirs, ours, truth)
    # the scatter as the gradient of the lookup it is the adjoint of
    g = grid0.double()[None, None].clone().requires_grad_(True)
    val = TR.pseudo_grad(z.double() * scale, depth.double()[:, None] * scale)
    OC.trilinear_lookup(g, pts.double()).backward(gradient=val)
    scattered = TR.trilinear_scatter(V, pts.double().reshape(-1, 3), val.reshape(-1))
    assert TR.block_err(scattered, g.grad[0, 0]) < 1e-12 * float(g.grad.abs().max())
    assert torch.equal(TR.pseudo_grad(z * scale, depth[:, None] * scale), OC.logits_pseudo_grad(z * scale, depth[:, None] * scale))


# ------------------------------------------------------------------------------------------- the generators keep their conditions
@pytest.mark.parametrize("seed", LIDAR_SEEDS)
def test_lidar_case_leaves_out_few_rays_and_reaches_every_face(seed):
    case = TR.lidar_case(seed)
    assert [int(k.sum()) for k in case["keep"]] == list(TR.LIDAR_KEPT)
    n_cand = sum(len(i) for i in case["idx"])
    assert sum(int(t.sum()) for t in case["tie"]) <= 0.02 * n_cand
    assert len({t.shape[1] for t in case["tables"]}) == len(case["tables"])          # every table has its own n_points
    far_range = case["ray_range"][1] / case["scale"]
    rec = TR.lidar_records(case, case["T"].double(), torch.float64)
    for s, k in enumerate(case["kept"]):
        idx = case["idx"][s][case["keep"][s]]
        assert not bool(TR.near_tie(rec[s], far_range).any())
        if k >= 63:
            assert len(torch.unique(idx)) < k                                        # drawn with repeats
            assert not bool(case["keep"][s].all())                                   # and the mask drops rays
        if k == 1000:
            face = TR.exit_face(rec[s], far_range)
            assert all(int((face == f).sum()) >= 20 for f in range(6)), (face + 1).bincount()
            assert 0.15 * k < int((face == -1).sum()) < 0.6 * k                       # about a third are range-limited
    assert len(case["idx"][0]) == 0 and len(case["idx"][-1]) > 0                      # an empty segment, and one emptied by the mask


def test_special_segments_are_what_they_claim():
    case = TR.lidar_case(SPECIAL_SEED, kept=(200, 200), special=("zero", "outside"))
    n_cand = sum(len(i) for i in case["idx"])
    assert sum(int(t.sum()) for t in case["tie"]) <= 0.02 * n_cand
    rec32 = TR.lidar_records(case, case["T"], torch.float32)
    assert float(rec32[0][:, 4].abs().max()) == 0.0                                   # a direction component exactly 0
    assert float(rec32[1][:, 0].min()) > 1.0                                          # origin outside the cube on x
    out = rec32[1][:, 3] > 0
    assert int(out.sum()) >= 20 and float(rec32[1][out, 12].abs().max()) == 0.0       # t_raw <= 0 on both x planes: far = 0
    assert int((rec32[1][:, 12] > 0).sum()) >= 20


def test_chain_case_and_update_generators():
    case = TR.chain_case(CHAIN_SEED)
    ang = case["pose6"][:, 3:6].double().norm(dim=1)
    assert torch.allclose(ang, torch.tensor(TR.CHAIN_ANGLES, dtype=torch.float64), rtol=1e-6, atol=0)
    assert sum(int(t.sum()) for t in case["tie"]) <= 0.02 * sum(len(i) for i in case["idx"])
    p, which = TR.pose_cases(0)
    ang = p[:, 3:6].double().norm(dim=1)
    want = torch.tensor(TR.POSE_ANGLES, dtype=torch.float64)[which]
    assert torch.allclose(ang, want, rtol=3e-7, atol=0)
    small = ang[which == TR.POSE_ANGLES.index(9.9e-7)], ang[which == TR.POSE_ANGLES.index(1.01e-6)]
    assert bool((small[0].float() < 1e-6).all()) and bool((small[1].float() > 1e-6).all())   # either side of the series switch, in float32 too
    assert bool((p.reshape(-1, 5, 6)[:, 4, 3:6] == 0).any(dim=1).all())                # one case per angle with a component exactly 0
    g = TR.log_uniform_grads(7000, torch.Generator().manual_seed(0))
    nz = g[g != 0].abs()
    assert bool((g[3::7] == 0).all()) and float(nz.min()) < 1e-11 and float(nz.max()) > 1e5
    for V, S, n in ((24, 100, 37), (100, 512, 16), (7, 64, 5)):
        rays, z, _ = TR.occ_batch(V, S, n, seed=5)
        pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
        outside = float((pts.abs() > 1).any(dim=-1).float().mean())
        assert 0.1 < outside < 0.35, outside
