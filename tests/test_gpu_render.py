"""render_forward, render_backward and los_loss_fused at the edges of every sample tier (C = 1 .. 32 samples per lane), against the
float64 truth of tests/render_restatement.py - needs an MI355X.

The cases are RR.case(S): 26 rays (7 workgroups, the last with two live waves) with an explicit noise tensor.  Every floating-point
check is made PER BLOCK against that block's own magnitude: a ray's weights against its largest weight times the transmittance's
growth, its depth, opacity and variance against what they are sums of (RR.forward_magnitudes), a ray's d_sigma against the terms it
is the difference of (M), its direction gradient against D, the far column against the far term (render_backward: per ray; the loss:
one block), a ray's mean / sd / js / eps against their conditioning, the five loss terms against the largest single ray's share times
the number of rays.  A block passes when its error is at most 4 x (the error of the oracle's float32 run on the CPU, same inputs, same
block) + 4 ulp of the block's magnitude; nothing is derived from the kernel's output.  "bit" is torch.equal; a result that is not
finite fails before anything is compared.

The fused loss is launched on the rays whose discrete decisions float32 cannot take the other way (RR.decided: at most 2 of 26 are
left out, otherwise the test fails) with the counts and far[0] of the whole batch, and once per S on all 26 rays for the outputs that
depend on no decision.  It has no case above 1024 samples: the library refuses them (tests/test_host.py).

Measured (CPU float32 noise | kernel on the MI355X, both relative to the block's magnitude, at the block that came closest to its
bound over all S, selections and cotangent sets; last column: that block's error as a fraction of its bound).  The CPU noise is that
of the machine the test ran on; the float32 run of another CPU differs from it by up to a factor of two on single blocks:

    check                                          CPU noise | kernel  of bound  (worst block)
    render_forward: weights                        7.76e-07 | 7.76e-07   0.22   (S = 63 ray 24)
    render_forward: depth                          3.65e-08 | 3.65e-08   0.06   (S = 64 ray 10)
    render_forward: opacity                        8.24e-08 | 8.24e-08   0.10   (S = 64 ray 10)
    render_forward: variance                       1.60e-07 | 1.59e-07   0.14   (S = 2 ray 11)
    render_backward (all): d_sigma                 1.88e-08 | 7.14e-08   0.13   (S = 2 ray 14)
    render_backward (all): d_rays directions       2.23e-08 | 1.13e-07   0.20   (S = 129 ray 0)
    render_backward (all): d_rays far              5.84e-08 | 5.84e-08   0.08   (S = 64 ray 10)
    render_backward (depth): d_sigma               1.99e-08 | 1.24e-07   0.22   (S = 63 ray 24)
    render_backward (depth): d_rays directions     1.63e-08 | 1.17e-07   0.22   (S = 63 ray 15)
    render_backward (depth): d_rays far            4.41e-08 | 4.41e-08   0.07   (S = 64 ray 10)
    render_backward (variance): d_sigma            1.37e-08 | 3.04e-07   0.57   (S = 512 ray 4)
    render_backward (variance): d_rays directions  8.77e-09 | 1.59e-07   0.31   (S = 512 ray 9)
    render_backward (variance): d_rays far         6.28e-09 | 3.73e-07   0.74   (S = 65 ray 8)
    loss: total term                               1.51e-07 | 1.28e-07   0.12   (S = 64 L2_JS)
    loss: depth term                               2.83e-08 | 4.25e-08   0.07   (S = 1024 L2_LOS)
    loss: los term                                 1.06e-06 | 1.20e-06   0.25   (S = 512 L2_JS)
    loss: opacity term                             2.22e-09 | 4.96e-08   0.10   (S = 1024 L2_LOS)
    loss: sum of eps term                          2.00e-08 | 3.40e-07   0.61   (S = 63 L2_JS)
    loss: d_sigma                                  9.36e-08 | 5.25e-07   0.62   (S = 128 L1_LOS ray 0)
    loss: d_rays directions                        1.73e-08 | 1.83e-07   0.33   (S = 63 L1_JS ray 3)
    loss: d_rays far                               2.15e-07 | 4.14e-07   0.31   (S = 512 L2_LOS)
    loss: weights                                  1.13e-07 | 2.27e-07   0.24   (S = 257 L2_LOS ray 6)
    loss: depth                                    3.65e-08 | 3.65e-08   0.06   (S = 64 L2_LOS ray 10)
    loss: opacity                                  8.24e-08 | 8.24e-08   0.10   (S = 64 L2_LOS ray 10)
    loss: variance                                 1.60e-07 | 1.59e-07   0.14   (S = 2 L2_LOS ray 11)
    loss: ray_stats mean                           1.01e-08 | 5.24e-08   0.10   (S = 65 L2_LOS ray 9)
    loss: ray_stats sd                             1.49e-07 | 1.47e-07   0.14   (S = 2 L2_LOS ray 11)
    loss: ray_stats js                             1.37e-07 | 1.35e-07   0.13   (S = 2 L2_LOS ray 11)
    loss: ray_stats eps                            9.09e-09 | 3.95e-08   0.08   (S = 513 L2_JS ray 17)
    loss, whole batch: weights                     1.13e-07 | 2.27e-07   0.24   (S = 257 ray 6)
    loss, whole batch: depth                       3.65e-08 | 3.65e-08   0.06   (S = 64 ray 10)
    loss, whole batch: opacity                     8.24e-08 | 8.24e-08   0.10   (S = 64 ray 10)
    loss, whole batch: variance                    1.60e-07 | 1.59e-07   0.14   (S = 2 ray 11)
"""
import pytest
import torch

from tests import render_restatement as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
PLUMBING_COUNTS = (63, 65, 129, 257, 513)                 # one ragged S per tier of the fused loss
ZERO_COLUMNS = [0, 1, 2, 6, 7, 8, 9, 10, 11]              # of d_rays: only the direction and far columns carry a gradient here


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


def _host(*tensors):
    """the kernel's outputs on the host; none of them may hold a NaN or an infinity (a NaN error would pass every `err > limit`)"""
    out = [t.cpu() for t in tensors]
    for t in out:
        assert bool(torch.isfinite(t).all())
    return out


def _inputs(c, rows=slice(None)):
    return [dv(c[k][rows]) for k in ("sigma", "z", "rays", "noise")]


def _check_forward(led, name, ref, rows, weights, depth, opacity, variance, where):
    """weights, depth, opacity and variance per ray"""
    f32, f64 = ref["f32"], ref["f64"]
    RR.check_rows(led, f"{name}: weights", weights, f32["weights"][rows], f64["weights"][rows], ref["weights_mag"][rows], where)
    for key, x in (("depth", depth), ("opacity", opacity), ("variance", variance)):
        RR.check_rows(led, f"{name}: {key}", x, f32[key][rows], f64[key][rows], ref["mag"][key][rows], where)


def _check_gradients(led, name, ref, g32, g64, rows, dens, d_sigma, d_rays, where, far_per_ray):
    """d_sigma rows against M, the direction columns per ray against D, the far column against the far term (render_backward: per ray,
    its far term carries each ray's own conditioning; the loss: one block); exact zeros elsewhere"""
    RR.check_rows(led, f"{name}: d_sigma", d_sigma, g32[0][rows], g64[0][rows], ref["M"][rows].max(1).values, where)
    RR.check_rows(led, f"{name}: d_rays directions", d_rays[:, 3:6], g32[1][rows, 3:6], g64[1][rows, 3:6], ref["D"][rows], where)
    if far_per_ray:
        RR.check_rows(led, f"{name}: d_rays far", d_rays[:, 12], g32[1][rows, 12], g64[1][rows, 12], ref["far_mag"][rows], where)
    else:
        RR.check_case(led, f"{name}: d_rays far", d_rays[:, 12], g32[1][rows, 12], g64[1][rows, 12], float(ref["far_mag"][rows].max()), where)
    assert torch.equal(d_rays[:, ZERO_COLUMNS], torch.zeros(d_rays.shape[0], len(ZERO_COLUMNS)))
    assert float(d_sigma[dens[rows] <= 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- a. render_forward
@pytest.mark.parametrize("S", RR.SAMPLE_COUNTS)
def test_render_forward_at_every_tier_edge(ops, S):
    c, ref = RR.case(S), RR.forward_reference(S)
    sigma, z, rays, noise = _inputs(c)
    depth, weights, opacity, variance = _host(*ops.render_forward(sigma, z, rays, noise=noise, noise_std=1.0))
    assert weights.shape == (RR.N_RAYS, S)
    led = RR.Ledger()
    _check_forward(led, "render_forward", ref, slice(None), weights, depth, opacity, variance, f"S = {S}")
    # without the weights: the same three scalars, bit for bit
    d2, w2, o2, v2 = ops.render_forward(sigma, z, rays, noise=noise, noise_std=1.0, want_weights=False)
    assert w2 is None and torch.equal(d2.cpu(), depth) and torch.equal(o2.cpu(), opacity) and torch.equal(v2.cpu(), variance)
    _finish(led)


# ------------------------------------------------------------------------------------------- b. render_backward
@pytest.mark.parametrize("which", RR.COTANGENT_SETS)
@pytest.mark.parametrize("S", RR.SAMPLE_COUNTS)
def test_render_backward_at_every_tier_edge(ops, S, which):
    c, ref = RR.case(S), RR.backward_reference(S, which)
    sigma, z, rays, noise = _inputs(c)
    cot = {k: (dv(v) if v is not None else None) for k, v in ref["cot"].items()}
    d_sigma, d_rays = _host(*ops.render_backward(sigma, z, rays, cot["depth"], cot["weights"], cot["opacity"], cot["variance"],
                                                 noise=noise, noise_std=1.0))
    assert d_sigma.shape == (RR.N_RAYS, S) and d_rays.shape == (RR.N_RAYS, 13)
    led = RR.Ledger()
    _check_gradients(led, f"render_backward ({which})", ref, ref["g32"], ref["g64"], slice(None), c["dens"], d_sigma, d_rays, f"S = {S}", far_per_ray=True)
    _finish(led)


# ------------------------------------------------------------------------------------------- c. los_loss_fused
def _loss_config(selection):
    from loner_amd import hip
    cfg = RR.loss_config(selection)
    return hip.LossConfig(selection=hip.LOSS_SELECTIONS[selection], min_js=cfg.min_js, max_js=cfg.max_js, js_alpha=cfg.js_alpha,
                          los_lambda=cfg.los_lambda, depth_lambda=RR.DEPTH_LAMBDA, min_eps=cfg.min_eps, fixed_eps=RR.FIXED_EPS)


def _launch_loss(ops, S, selection, rows, n_rays_dev=None):
    """the fused loss on the rays `rows` of the case with the normalisers and far[0] of the whole batch -> its five outputs"""
    assert S <= RR.LOSS_MAX_SAMPLES
    c, ref = RR.case(S), RR.loss_reference(S, selection)
    sigma, z, rays, noise = _inputs(c, rows)
    counts = torch.tensor(ref["counts"], dtype=torch.int32, device=DEV)
    far0 = dv(ref["far0"].reshape(1))
    live = None if n_rays_dev is None else torch.tensor([n_rays_dev], dtype=torch.int32, device=DEV)
    return ops.los_loss_fused(sigma, z, rays, dv(c["depth_gt"][rows]), RR.SCALE, _loss_config(selection), counts, noise=noise, noise_std=1.0,
                              n_rays_dev=live, want_stats=True, want_weights=True, far0=far0)


@pytest.mark.parametrize("selection", RR.SELECTIONS)
@pytest.mark.parametrize("S", RR.LOSS_SAMPLE_COUNTS)
def test_los_loss_fused_on_the_decided_rays(ops, S, selection):
    c, ref, fwd = RR.case(S), RR.loss_reference(S, selection), RR.forward_reference(S)
    keep = ref["decided"]
    assert int((~keep).sum()) <= 2, f"more than 2 of {RR.N_RAYS} rays are undecided: {torch.nonzero(~keep)[:, 0].tolist()}"
    loss_out, d_sigma, d_rays, stats, weights = _host(*_launch_loss(ops, S, selection, keep))
    n = int(keep.sum())
    assert d_sigma.shape == (n, S) and d_rays.shape == (n, 13) and stats.shape == (n, 8) and weights.shape == (n, S)
    where = f"S = {S} {selection}"
    led = RR.Ledger()
    t32, t64 = RR.loss_terms(S, selection, keep, F32), RR.loss_terms(S, selection, keep, F64)
    for k, (term, mag) in enumerate(zip(("total", "depth", "los", "opacity", "sum of eps"), RR.loss_term_magnitudes(ref, keep))):
        led.figures(f"loss: {term} term", abs(float(loss_out[k]) - float(t64[k])), abs(float(t32[k]) - float(t64[k])), max(mag, abs(float(t64[k]))), where)
    g32, g64 = (ref["r32"]["d_sigma"], ref["r32"]["d_rays"]), (ref["r64"]["d_sigma"], ref["r64"]["d_rays"])
    _check_gradients(led, "loss", ref, g32, g64, keep, c["dens"], d_sigma, d_rays, where, far_per_ray=False)
    _check_forward(led, "loss", fwd, keep, weights, stats[:, 0], stats[:, 1], stats[:, 2], where)
    RR.check_statistics(led, stats[:, 3:7], ref, keep, where, prefix="loss: ray_stats ")
    if selection.endswith("LOS"):
        assert torch.equal(stats[:, 6], torch.full((n,), RR.FIXED_EPS))                  # js selects nothing: the configured margin, bit for bit
    assert torch.equal(stats[:, 7], ref["opaque"][keep].float())
    _finish(led)


@pytest.mark.parametrize("S", RR.LOSS_SAMPLE_COUNTS)
def test_los_loss_fused_whole_batch_renders_like_the_forward(ops, S):
    """all 26 rays: weights_out and ray_stats[:, 0:3] depend on none of the loss's decisions, and the opaque flag only on depth_gt"""
    ref, fwd = RR.loss_reference(S, "L1_JS"), RR.forward_reference(S)
    _, _, _, stats, weights = _host(*_launch_loss(ops, S, "L1_JS", slice(None)))
    led = RR.Ledger()
    _check_forward(led, "loss, whole batch", fwd, slice(None), weights, stats[:, 0], stats[:, 1], stats[:, 2], f"S = {S}")
    assert torch.equal(stats[:, 7], ref["opaque"].float())
    _finish(led)


# ------------------------------------------------------------------------------------------- d. plumbing
@pytest.mark.parametrize("S", PLUMBING_COUNTS)
def test_los_loss_fused_is_deterministic_and_honours_the_device_ray_count(ops, S):
    first = [t.cpu() for t in _launch_loss(ops, S, "L1_JS", slice(None))]
    again = [t.cpu() for t in _launch_loss(ops, S, "L1_JS", slice(None))]
    for a, b in zip(first, again):                                                      # loss_out included: the block-partial reduction
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    live = 17
    short = [t.cpu() for t in _launch_loss(ops, S, "L1_JS", slice(0, live))]
    part = [t.cpu() for t in _launch_loss(ops, S, "L1_JS", slice(None), n_rays_dev=live)]
    assert torch.equal(part[0].view(torch.int32), short[0].view(torch.int32))           # loss_out
    for a, b in zip(part[1:], short[1:]):
        assert torch.equal(a[:live].view(torch.int32), b.view(torch.int32))
    assert torch.equal(part[2][live:], torch.zeros(RR.N_RAYS - live, 13))               # d_rays behind the live rows
    assert not torch.equal(short[0], first[0])                                           # fewer rays: another loss
