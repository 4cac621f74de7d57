"""The keyframe-sharded optimisation loop (loner_amd/mapping/sharding.py + Optimizer.set_distributed) with the real HIP
kernels on the one GPU of the test box.

* RCCL (`backend="nccl"`) at world_size 1: the collectives of the sharded loop (the front-record all-gather that carries far[0]
  and the loss normalisers, the density gradient exchange, the occupancy pseudo-gradient) execute on the device through RCCL
  and the run is bit-identical to the non-distributed one.
* FOUR processes sharing the GPU over gloo on the DEFAULT network (2^18-entry tables, 7.4 M parameters): the BASELINE configs[3]
  window - 8 keyframes, two per rank, the default `reduce_scatter` exchange (4 chunks, ranged Adam, all-gather) - and a
  2-keyframe window with two idle ranks.  (At most five processes hold the GPU at once: the test process and four ranks.)
* two / three processes sharing the GPU over gloo (RCCL refuses several ranks on one device; the torch.distributed calls
  are the same): replicas end bit-identical, only a rank's own non-anchored keyframes move, a rank that owns no keyframe
  (window smaller than the world size) still joins every collective, and - on identical, keyframe-keyed random draws -
  the sharded loss trace and parameters equal the single-GPU run's (incl. the reference's far[0] quirk, whose far value is
  broadcast from rank 0).
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N_RAYS, N_SAMPLES = 128, 64
BIG_RAYS, BIG_SAMPLES = 512, 512          # the 4-rank runs on the default network: BASELINE configs[3]'s per-GPU shape, 512 rays x 512 samples


class KeyedDraws:
    """Random draws in the reference's order that depend only on (iteration, GLOBAL keyframe index), so that a
    rank owning keyframes `owned` of the window draws exactly what a single process draws for those keyframes.  Requires that
    no candidate ray is dropped (then row i of the compacted batch is candidate i)."""

    def __init__(self, owned, n_rays=N_RAYS):
        self.owned, self.n_rays = list(owned), n_rays
        self.calls = 0

    def _gen(self, it, kf, kind):
        return torch.Generator().manual_seed(1_000_003 * it + 1_009 * kf + kind)

    def _it(self):
        return self.calls // len(self.owned)

    def ray_index(self, n_points, count):
        kf = self.owned[self.calls % len(self.owned)]
        idx = torch.randint(0, n_points, (count,), generator=self._gen(self._it(), kf, 0))
        self.calls += 1
        return idx

    def _per_kf(self, kind, width, normal=False):
        it = (self.calls - 1) // len(self.owned)
        f = torch.randn if normal else torch.rand
        return torch.cat([f(self.n_rays, width, generator=self._gen(it, kf, kind)) for kf in self.owned])

    def jitter(self, n, h): return self._per_kf(1, h)
    def pdf(self, n, h): return self._per_kf(2, h)
    def noise(self, n, s): return self._per_kf(3, s, normal=True)


def _poses(n_kf):
    """window poses: the anchored first keyframe exact, the others offset by a few centimetres (something to optimise)"""
    from loner_amd.utils import synthetic as SY
    base = SY.trajectory_pose6(n_kf)
    poses = [base[0].clone()] + [p.clone() + torch.tensor([0.03, -0.02, 0.01, 0.0, 0.0, 0.0]) for p in base[1:]]
    return poses


def _setup(world_window, seed=0, default_net=False):
    from tests.test_gpu_mapping import make_keyframes, small_settings, world_cube
    from loner_amd.mapping.optimizer import Optimizer
    torch.cuda.set_device(0)
    if default_net:
        from loner_amd.common.settings import default_optimizer_settings
        s = default_optimizer_settings()
        s["num_samples"]["lidar"], s["num_samples"]["sky"] = BIG_RAYS, 0
        s["model_config"]["model"]["render"]["N_samples_train"] = BIG_SAMPLES
    else:
        s = small_settings(N_RAYS, N_SAMPLES)
    torch.manual_seed(seed)                                 # identical initial parameters on every rank
    opt = Optimizer(s, None, world_cube(), 0, False, True, False)
    if default_net:
        # Features of order one instead of the initialiser's 1e-4.  With tables at 1e-4 and Adam steps of 1e-2 the first iterations are
        # chaotic - every touched entry jumps by 100x its value, ReLU boundaries flip on a last-bit difference of the gradient sum, and
        # two CORRECT runs that differ only in summation order (one fixed-point total against the fp32 sum of eight) are 1e-2 apart
        # after 7 iterations (measured: 1.4 % of the entries off by > 1e-3 after 4 iterations, 31 % after 7) - which would hide a
        # wrong exchange behind a loose tolerance.  Scaled tables put the comparison where differences stay differences.
        sig = opt._model.nerf_model._model_sigma
        with torch.no_grad():
            sig.params[int(sig.spec.n_mlp_params):] *= 3000.0
    window = make_keyframes(_poses(world_window))
    window[0].is_anchored = True
    return opt, window


def _blobs(opt):
    params = opt._model.nerf_model._model_sigma.params
    st = opt._optimizer.state[params]
    return [params.detach(), st["exp_avg"], st["exp_avg_sq"], opt._occupancy_grid_model.occupancy_grid.detach().reshape(-1)]


def _worker(rank, world, port, ret, backend, n_kf, n_it, keyed, exchange="all_reduce", payload="fp32", default_net=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from loner_amd.mapping.optimizer import OptimizationSettings
    from loner_amd.mapping.sharding import DistContext, shard_window
    opt, window = _setup(n_kf, default_net=default_net)
    ctx = DistContext(exchange=exchange, payload=payload)
    opt.set_distributed(ctx)
    owned_ids = shard_window(n_kf, world, rank)
    if keyed:
        if owned_ids:
            opt.set_draws(KeyedDraws(owned_ids, n_rays=BIG_RAYS if default_net else N_RAYS))
    else:
        torch.manual_seed(100 + rank)                       # different ray draws per rank
    before = [kf.get_lidar_pose().get_pose_tensor().detach().clone() for kf in window]
    opt._do_iterate_optimizer(window, [None], optimizer_settings=OptimizationSettings(n_it, False, False, False, True))
    torch.cuda.synchronize()
    blobs = _blobs(opt)
    sums = torch.stack([b.double().sum() for b in blobs] + [b.double().abs().sum() for b in blobs]).cpu()
    gathered = [torch.zeros_like(sums) for _ in range(world)]
    dist.all_gather(gathered, sums if backend != "nccl" else sums.cuda())
    # the loss of the whole window = sum of the ranks' partial sums (each already normalised by the GLOBAL counts)
    loss = opt.last_stats["loss_terms"][:, :4].double().cpu()
    if backend == "nccl":
        loss = loss.cuda()
    dist.all_reduce(loss)
    moved = [float((kf.get_lidar_pose().get_pose_tensor().detach() - b).abs().max()) for kf, b in zip(window, before)]
    ret[rank] = dict(sums=[g.cpu().tolist() for g in gathered], loss=loss.cpu().numpy(), finite=bool(torch.isfinite(blobs[0]).all()),
                     moved=moved, owned=owned_ids, step=opt._global_step,
                     # (default network: 30 MB per rank through the manager - the first and the last rank hand theirs over, the
                     # replicas are compared by the gathered sums)
                     params=blobs[0].cpu().numpy() if (not default_net or rank in (0, world - 1)) else None,
                     grid=blobs[3].cpu().numpy(), poses=[kf.get_lidar_pose().get_pose_tensor().detach().cpu().numpy() for kf in window],
                     n_valid=opt.last_stats["n_valid_rays"], adam_steps=opt._optimizer.state[opt._model.nerf_model._model_sigma.params]["step"],
                     exchange=ctx.exchange, owned_range=ctx.owned_range(blobs[0].numel()))
    if default_net:
        # the exchange itself at this world size on the device tensors of the default network, against a closed form: rank r contributes
        # (r + 1) everywhere and i mod 7 on top; zero_rest=False is the training loop's form (the rest keeps the rank's own values)
        n = blobs[0].numel()
        ramp = (torch.arange(n, device="cuda") % 7).float()
        flat = ramp + float(rank + 1)
        ctx.exchange_grads(flat, async_op=True, zero_rest=False).wait()
        total = world * ramp + float(world * (world + 1) // 2)
        sl = ctx.owned_range(n)
        if sl is None:
            ok = bool(torch.equal(flat, total))
        else:
            ok = bool(torch.equal(flat[sl[0]:sl[1]], total[sl[0]:sl[1]])) and bool(torch.equal(flat[:sl[0]], (ramp + float(rank + 1))[:sl[0]]))
            ctx.gather_params(flat)
            ok = ok and bool(torch.equal(flat, total))
        ret[rank] = dict(ret[rank], exchange_exact=ok)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, backend, n_kf, n_it, keyed, exchange="all_reduce", payload="fp32", default_net=False, timeout=300):
    port = 29600 + (os.getpid() * 7 + world * 13 + n_kf) % 300
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret, backend, n_kf, n_it, keyed, exchange, payload, default_net)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout)
            assert p.exitcode == 0, "a rank of the sharded run failed (or deadlocked)"
    finally:
        # a rank that failed leaves its peers waiting in a collective: none of them may outlive the test with the GPU open
        for q in procs:
            if q.is_alive():
                q.kill()
            q.join()
    return [ret[r] for r in range(world)]


def _single(n_kf, n_it, keyed, default_net=False):
    from loner_amd.mapping.optimizer import OptimizationSettings
    opt, window = _setup(n_kf, default_net=default_net)
    if keyed:
        opt.set_draws(KeyedDraws(list(range(n_kf)), n_rays=BIG_RAYS if default_net else N_RAYS))
    opt._do_iterate_optimizer(window, [None], optimizer_settings=OptimizationSettings(n_it, False, False, False, True))
    torch.cuda.synchronize()
    blobs = _blobs(opt)
    return dict(loss=opt.last_stats["loss_terms"][:, :4].double().cpu().numpy(), params=blobs[0].cpu().numpy(), grid=blobs[3].cpu().numpy(),
                poses=[kf.get_lidar_pose().get_pose_tensor().detach().cpu().numpy() for kf in window], n_valid=opt.last_stats["n_valid_rays"],
                blobs=[b.clone() for b in blobs])


def test_two_ranks_one_gpu_replicas_stay_identical():
    r0, r1 = _run(2, "gloo", 4, 25, keyed=False)
    assert r0["sums"][0] == r0["sums"][1] == r1["sums"][0] == r1["sums"][1]      # bit-identical replicas (sum and |sum| of each blob)
    for r in (r0, r1):
        assert r["finite"] and r["step"] == 25 and r["adam_steps"] == 25 and r["loss"][-1, 0] < r["loss"][0, 0]
        for k, moved in enumerate(r["moved"]):
            assert (moved > 0) == (k in r["owned"] and k != 0)          # only this rank's non-anchored keyframes move
    assert r0["owned"] == [0, 2] and r1["owned"] == [1, 3]


def test_sharded_run_equals_single_gpu_on_identical_draws():
    """2 ranks vs 1 process on the same (keyframe-keyed) random draws, 12 iterations incl. two occupancy steps: the window loss
    of every iteration, the final parameters, occupancy grid and poses agree.  Not bit-equal: the density gradient is the fp32
    sum of two per-rank fixed-point totals instead of one, a last-bit difference per entry that Adam carries along."""
    n_it = 12
    single = _single(4, n_it, keyed=True)
    r0, r1 = _run(2, "gloo", 4, n_it, keyed=True)
    assert single["n_valid"] == n_it * 4 * N_RAYS and r0["n_valid"] + r1["n_valid"] == single["n_valid"]   # no ray dropped: draws line up
    assert r0["sums"][0] == r0["sums"][1]
    rel_loss = np.abs(r0["loss"] - single["loss"]).max(axis=0) / np.abs(single["loss"]).max(axis=0)
    print("sharded vs single: loss terms rel", rel_loss, " params rel", np.abs(r0["params"] - single["params"]).max() / np.abs(single["params"]).max())
    assert np.abs(r0["loss"][0] - single["loss"][0]).max() <= 2e-6 * np.abs(single["loss"][0]).max()      # first iteration: same parameters
    assert rel_loss.max() < 2e-4
    assert np.abs(r0["params"] - single["params"]).max() < 2e-4 * np.abs(single["params"]).max()
    assert np.abs(r0["grid"] - single["grid"]).max() < 1e-3 * max(np.abs(single["grid"]).max(), 1e-12)
    for k in range(4):
        owner = r0 if k % 2 == 0 else r1
        assert np.abs(owner["poses"][k] - single["poses"][k]).max() < 2e-5


def test_reduce_scatter_exchange_and_bf16_payload():
    """The sharded-Adam form of the exchange (reduce-scatter of the flat gradient in equal chunks, Adam on a rank's own chunk,
    all-gather of the stepped chunks) gives the bits of the all-reduce form - with two ranks a sum has one order -
    and its replicas stay identical.  The bf16 payload halves the bytes on the wire: replicas identical among themselves, the
    map within bf16 rounding of the fp32 run's."""
    n_it = 12
    ar = _run(2, "gloo", 4, n_it, keyed=True)
    rs = _run(2, "gloo", 4, n_it, keyed=True, exchange="reduce_scatter")
    same_map = lambda sums: all([s_[i] for i in (0, 3, 4, 7)] == [sums[0][i] for i in (0, 3, 4, 7)] for s_ in sums)   # parameters and grid
    assert same_map(rs[0]["sums"])                  # (the Adam moments of a chunk live on the rank that steps it)
    assert np.array_equal(rs[0]["params"], ar[0]["params"]) and np.array_equal(rs[1]["params"], ar[1]["params"])
    assert np.array_equal(rs[0]["loss"], ar[0]["loss"]) and np.array_equal(rs[0]["grid"], ar[0]["grid"])
    for mode in ("all_reduce", "reduce_scatter"):
        bf = _run(2, "gloo", 4, n_it, keyed=True, exchange=mode, payload="bf16")
        assert same_map(bf[0]["sums"])                                                       # replicas never drift
        assert np.abs(bf[0]["loss"][0] - ar[0]["loss"][0]).max() <= 1e-6 * np.abs(ar[0]["loss"][0]).max()    # first iteration: same map
        rel_loss = np.abs(bf[0]["loss"] - ar[0]["loss"]).max() / np.abs(ar[0]["loss"]).max()
        print(f"bf16 payload ({mode}): loss trace vs fp32 payload rel {rel_loss:.2e}")
        assert rel_loss < 5e-2 and bf[0]["loss"][-1, 0] < bf[0]["loss"][0, 0]


def test_rank_without_keyframes_joins_every_collective():
    """window (2 keyframes) smaller than the world (3 ranks): rank 2 owns nothing, must neither crash nor deadlock, and ends
    with the same replica; the result equals the single-process run on the same draws."""
    n_it = 11
    single = _single(2, n_it, keyed=True)
    rs = _run(3, "gloo", 2, n_it, keyed=True)
    assert [r["owned"] for r in rs] == [[0], [1], []]
    assert rs[0]["sums"][0] == rs[0]["sums"][1] == rs[0]["sums"][2]
    assert all(r["step"] == n_it and r["adam_steps"] == n_it for r in rs)
    assert np.abs(rs[2]["params"] - single["params"]).max() < 2e-4 * np.abs(single["params"]).max()
    assert np.abs(rs[0]["loss"] - single["loss"]).max() < 2e-4 * np.abs(single["loss"]).max()
    # the same with the reduce-scatter exchange: the small net's 26624 parameters do not split into three aligned chunks -> it must
    # fall back to the all-reduce form rather than fail
    rs3 = _run(3, "gloo", 2, n_it, keyed=True, exchange="reduce_scatter")
    assert rs3[0]["sums"][0] == rs3[0]["sums"][1] == rs3[0]["sums"][2]                      # (fallback: moments replicated too)
    assert np.array_equal(rs3[0]["params"], rs[0]["params"])


def test_front_record_kernels_equal_their_torch_forms():
    """lnr_shard_front_pack / lnr_shard_front_reduce (the sharded loop's one small collective: far[0] and both loss normalisers from an
    all-gather of {first-ray key, live count, depths}) against the plain-torch forms the CPU gloo tests run, bit for bit: ragged
    segments, an empty first segment, a rank without keyframes, a live count below the buffer size, transparent rays on both sides."""
    from loner_amd import ops
    from loner_amd.mapping import sharding as SH
    gen = torch.Generator().manual_seed(4)
    cap, recs_k, recs_t = 700, [], []
    for r, (seg, order, n_live) in enumerate([([0, 0, 300, 640], [1, 4, 6], 600), ([0, 512], [2], 512), (None, None, 0), ([0, 5, 5], [0, 9], 5)]):
        if seg is None:
            recs_k.append(ops.shard_front_pack(None, None, (), None, None, cap, device="cuda"))
            recs_t.append(SH.front_record(None, None, (), None, 0, cap, device="cuda"))
            continue
        n = seg[-1]
        rays = torch.randn(n, 13, generator=gen)
        rays[:, 12] = 0.3 + 0.05 * r + 0.2 * torch.rand(n, generator=gen)
        depths = torch.rand(n, generator=gen) * 0.8 - 0.05                    # some non-positive, some beyond far
        seg_dev = torch.tensor(seg, dtype=torch.int32, device="cuda")
        n_dev = torch.tensor([n_live], dtype=torch.int32, device="cuda")
        recs_k.append(ops.shard_front_pack(rays.cuda(), seg_dev, order, depths.cuda(), n_dev, cap))
        recs_t.append(SH.front_record(rays.cuda(), seg_dev, order, depths.cuda(), n_dev, cap))
    for a, b in zip(recs_k, recs_t):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    allk = torch.cat(recs_k)
    counts_k, far0_k = ops.shard_front_reduce(allk, 4, 4 + cap)
    counts_t, far0_t = SH.reduce_front_records(allk, 4, 4 + cap)
    assert counts_k.tolist() == counts_t.tolist() and torch.equal(far0_k.view(torch.int32), far0_t.view(torch.int32))
    assert counts_k[0].item() == 600 + 512 + 0 + 5 and 0 < counts_k[1].item() < counts_k[0].item()
    # the batch's first ray is rank 3's (window position 0): every depth is compared with ITS far
    assert float(far0_k) == float(recs_k[3][0:1].view(torch.float32)) and float(far0_k) != float(recs_k[0][0:1].view(torch.float32))
    nobody = torch.cat([recs_k[2], recs_k[2]])
    c0, f0 = ops.shard_front_reduce(nobody, 2, 4 + cap)
    assert c0.tolist() == [0, 0] and bool(torch.isnan(f0).all())


def test_four_ranks_default_network_reduce_scatter_equals_single_gpu():
    """BASELINE configs[3]'s 8-keyframe window as far as one GPU can execute it: sharded two keyframes per rank over FOUR processes
    (gloo between them; every rank runs the HIP kernels on the shared MI355X), default network (16 x 2^18-entry levels, 7.4 M
    parameters), the exchange left at its default - `reduce_scatter` from 4 ranks: four 1 854 208-float chunks, ranged Adam, all-gather -
    3 iterations incl. the occupancy step at global step 0 (the L1 line-of-sight loss has a sign() in its gradient and Adam's steps are
    sign-sized: two CORRECT runs that differ in summation order drift apart by a factor ~5 per iteration - 0.7 % of the entries are off
    by > 1e-3 after 4 iterations, 32 % after 6, measured - so the comparison is made early, and the exchange is ALSO checked directly
    against a closed form on the same 4 ranks and device tensors).  On keyframe-keyed draws the window's loss trace, the final parameters,
    the grid and the poses equal the single-GPU run; the replicas are identical; every rank stepped exactly its chunk."""
    n_it, G = 3, 4
    single = _single(8, n_it, keyed=True, default_net=True)
    rs = _run(G, "gloo", 8, n_it, keyed=True, exchange=None, default_net=True, timeout=900)
    assert [r["owned"] for r in rs] == [[k, k + G] for k in range(G)] and all(r["exchange"] == "reduce_scatter" for r in rs)
    n_par = single["params"].size
    assert n_par == 7416832 and [r["owned_range"] for r in rs] == [(k * n_par // G, (k + 1) * n_par // G) for k in range(G)]
    assert single["n_valid"] == n_it * 8 * BIG_RAYS and sum(r["n_valid"] for r in rs) == single["n_valid"]       # no ray dropped: draws line up
    same_map = lambda sums: all([s_[i] for i in (0, 3, 4, 7)] == [sums[0][i] for i in (0, 3, 4, 7)] for s_ in sums)   # parameters and grid
    assert all(same_map(r["sums"]) for r in rs) and np.array_equal(rs[-1]["params"], rs[0]["params"])
    assert all(r["finite"] and r["step"] == n_it and r["adam_steps"] == n_it for r in rs)
    loss, ref = rs[0]["loss"], single["loss"]
    rel_loss = np.abs(loss - ref).max(axis=0) / np.abs(ref).max(axis=0)
    # parameters: Adam's first steps are sign-sized (lr = 1e-2) for every entry a gradient reaches, so the few entries whose gradient is
    # rounding-sized step differently on any change of summation order (the gradient here is the fp32 sum of four per-rank totals): a
    # quantile statement, as for the reference's own first iterations (G14).  A wrong exchange (a missing or doubled contribution)
    # changes m / sqrt(v) of most touched entries by a visible fraction of a step.
    dp = np.abs(rs[0]["params"] - single["params"])
    print("4 ranks vs single GPU: loss terms rel", rel_loss, " params: max", dp.max(), "99.9 % quantile", np.quantile(dp, 0.999), "fraction > 1e-3", (dp > 1e-3).mean())
    assert np.abs(loss[0] - ref[0]).max() <= 2e-6 * np.abs(ref[0]).max()            # first iteration: same parameters, same draws
    # (measured on eight ranks, one keyframe each, at configs[3]'s real per-GPU shape, 512 rays x 512 samples: loss terms within 1.4e-3,
    # 99 % of the 7.4 M entries within 3.5e-4, 0.2 % beyond 1e-3, max 1.3e-2; at 512 x 128 - rounds 4-5 - the 99 % quantile was below
    # 1e-4: four times the samples reach four times the entries whose first gradients are rounding-sized)
    assert rel_loss.max() < 2e-3 and np.quantile(dp, 0.99) < 1e-3 and (dp > 1e-3).mean() < 1e-2 and dp.max() <= 2.001e-2 * n_it
    assert all(r["exchange_exact"] for r in rs)                  # reduce-scatter + all-gather of 4 x 1 854 208 floats: the exact sums
    assert np.abs(rs[0]["grid"] - single["grid"]).max() < 1e-3 * max(np.abs(single["grid"]).max(), 1e-12)
    for k in range(8):
        assert np.abs(rs[k % G]["poses"][k] - single["poses"][k]).max() < 5e-4   # (three Adam steps of 1e-3 each; measured 2.0e-4 at 512 x 512, 2.1e-5 at 512 x 128)
    for r, res in enumerate(rs):
        assert all((res["moved"][j] > 0) == (j % G == r and j != 0) for j in range(8))       # only a rank's own non-anchored keyframes move


def test_four_ranks_two_keyframes_two_idle_ranks():
    """A 2-keyframe window on 4 ranks (the first keyframes of every run): ranks 2-3 own nothing, join every collective with an empty
    front record and a zero gradient, step their chunk of the parameters like everyone else and end with the same replica."""
    n_it, G = 3, 4
    single = _single(2, n_it, keyed=True, default_net=True)
    rs = _run(G, "gloo", 2, n_it, keyed=True, exchange=None, default_net=True, timeout=900)
    assert [r["owned"] for r in rs] == [[0], [1], [], []] and all(r["exchange"] == "reduce_scatter" for r in rs)
    same_map = lambda sums: all([s_[i] for i in (0, 3, 4, 7)] == [sums[0][i] for i in (0, 3, 4, 7)] for s_ in sums)   # parameters and grid
    assert all(same_map(r["sums"]) for r in rs) and np.array_equal(rs[-1]["params"], rs[0]["params"])
    assert all(np.array_equal(r["grid"], rs[0]["grid"]) for r in rs)
    assert all(r["step"] == n_it and r["adam_steps"] == n_it and r["finite"] for r in rs)
    assert np.abs(rs[0]["loss"] - single["loss"]).max() < 2e-3 * np.abs(single["loss"]).max() and all(r["exchange_exact"] for r in rs)
    dp = np.abs(rs[-1]["params"] - single["params"])                  # (a quantile statement: see the 8-keyframe test)
    print("2 keyframes on 4 ranks vs single GPU: params max", dp.max(), "99.9 % quantile", np.quantile(dp, 0.999), "fraction > 1e-3", (dp > 1e-3).mean())
    assert np.quantile(dp, 0.99) < 1e-4 and (dp > 3e-4).mean() < 2e-2 and dp.max() <= 2.001e-2 * n_it


def test_rccl_world_size_one_is_bit_identical_to_non_distributed():
    """backend "nccl" IS RCCL on ROCm: the sharded loop's collectives run on the device; with one rank they are identities."""
    n_it = 11
    single = _single(2, n_it, keyed=True)
    (r,) = _run(1, "nccl", 2, n_it, keyed=True)
    assert r["step"] == n_it
    assert np.array_equal(r["params"], single["params"]) and np.array_equal(r["grid"], single["grid"])
    assert np.array_equal(r["loss"], single["loss"])
    for a, b in zip(r["poses"], single["poses"]):
        assert np.array_equal(a, b)


def test_rccl_world_size_one_reduce_scatter_exchange_through_the_own_binding():
    """The `reduce_scatter` exchange at RCCL world size 1 - reduce-scatter of the flat gradient, ranged Adam step, IN-PLACE all-gather of
    the stepped chunk, all through lnr_comm_* (the library's own RCCL binding: DistContext picks it on the "nccl" backend) - is
    bit-identical to the non-distributed run as well; and the binding's collectives are identities on every dtype it moves."""
    n_it = 6
    single = _single(2, n_it, keyed=True)
    (r,) = _run(1, "nccl", 2, n_it, keyed=True, exchange="reduce_scatter")
    assert r["step"] == n_it and r["exchange"] == "reduce_scatter"
    assert np.array_equal(r["params"], single["params"]) and np.array_equal(r["grid"], single["grid"]) and np.array_equal(r["loss"], single["loss"])


def test_bench_entry_point_spawns_its_ranks_and_reports_what_the_group_saw():
    """`python bench.py --gpus 2` (no launcher around it) on the one GPU of the box, ranks over gloo: the line's n_gpus is the
    process group's world size and the sharded window trains (the driver's SCALE runs use this entry point with RCCL)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LNR_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--keyframes", "4",
                        "--rays", "128", "--samples", "128", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    assert line["config"]["parallelism"] == "keyframe-sharded x2"
