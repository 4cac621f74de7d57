"""tests/render_restatement.py checked without a GPU: its float64 autograd against central finite differences, its float64 run against
the recorded reference (goldens g5_render, g8_compute_loss), the conditions its cases promise to a comparison of the kernels with
them, and that the yardstick sees the slips it is for.

Conditions, as counted for the committed cases (seed 0 at every S; 26 rays: 17 opaque, 5 transparent, 4 without a return):

    S      undecided rays (L1_JS L2_JS L1_LOS L2_LOS)    rays with js < min_js | between | > max_js
    2      0 0 0 0                                        0 |  4 | 22
    63     0 0 0 0                                        5 | 11 | 10
    64     0 0 0 0                                        6 | 13 |  7
    65     0 0 0 0                                       10 | 11 |  5
    128    0 0 1 1                                       11 |  9 |  6
    129    0 0 0 0                                        7 | 13 |  6
    256    1 1 0 0                                        9 | 12 |  5
    257    0 0 0 0                                       12 |  9 |  5
    512    2 2 0 0                                        7 | 13 |  6
    513    1 1 0 0                                        8 | 13 |  5
    1000   0 0 1 1                                       10 | 11 |  5
    1024   0 0 0 0                                       10 | 12 |  4
    1025   0 0 1 1                                        9 | 13 |  4
    2047   0 0 0 0                                       12 | 10 |  4
    2048   0 0 1 1                                       10 | 12 |  4

Statistics (ray_stats columns 3..6) and the per-ray scalars depth, opacity, variance: the oracle's own float32 run, and a float32 run
of the restatement whose exponential leans by 2^-23 of its value at every sample, stay inside 4 ulp of `statistics_magnitudes` and
`forward_magnitudes` alone on every decided ray (statistics, largest: 0.31 of it, sd of ray 11 at S = 2, and 0.62 for the leaning
run, sd of ray 18 at S = 64; scalars: 0.09 and 0.51).  Slips (f) to (h) of `ray_statistics` each miss at every tier - (f) and (g) in sd
and js under every selection, (h) in eps under the JS selections.  (a) to (e) are judged as before; the far column of render_backward
now against the wider far term of `kernel_G_render` (one block per case here, per ray on the GPU), which (d) still misses.

Slips: every one of (a) to (e) misses the bound of at least one block at every tier.  (e) can only show at a ragged S (there is no
padding slot at S = 64 C) and only on a ray whose target window reaches depth 0: ray 3 of every case (surface at 1.7 m) under the
LOS selections (margin 2.57 m), and under the JS selections only where js gives that ray a margin above its depth (S = 63, 129, 257
of the six ragged S used here; not 65, 513, 1025).  It moves d_sigma only where a sample of positive density lies inside
that window (and under an L1 selection only where it turns the sign of w - target), which a case of 63 samples need not have: the
block it is asserted to miss is the los term of loss_out."""
import pytest
import torch

from oracle import network as NW
from oracle import render as ORD
from tests import render_restatement as RR
from tests.conftest import load_golden

F32, F64 = torch.float32, torch.float64
SLIP_COUNTS = (63, 65, 129, 257, 513, 1025)          # one ragged S per tier C = 1 .. 32
LOSS_SLIP_COUNTS = tuple(S for S in SLIP_COUNTS if S <= RR.LOSS_MAX_SAMPLES)      # the tiers the fused loss has


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------- the restatement is what it says
@pytest.mark.parametrize("dtype", [F32, F64])
def test_forward_and_loss_compute_in_the_dtype_they_are_given(dtype):
    c = RR.case(100)
    dens, z, rays, dgt = (c[k].to(dtype) for k in ("dens", "z", "rays", "depth_gt"))
    out = RR.forward(dens, z, rays)
    assert all(v.dtype == dtype for v in out.values())
    for sel in RR.SELECTIONS:
        r = RR.loss_run(dens, z, rays, dgt, sel)
        assert r["loss"].dtype == dtype and r["d_sigma"].dtype == dtype and r["d_rays"].dtype == dtype
        assert all(t.dtype == dtype for t in r["terms"])
        assert all(r["aux"][k].dtype == dtype for k in ("mean", "std", "js", "target"))
        assert RR.eps_of(r["aux"], RR.N_RAYS, dtype).dtype == dtype


@pytest.mark.parametrize("S", [7, 100, 513])
def test_parts_and_manual_backward_are_the_oracle_and_its_autograd(S):
    """ray_parts is composite; G of kernel_G_render / loss_pieces is the total derivative; manual_backward is autograd - to float64
    rounding of the term magnitudes; and |d_sigma| <= M elementwise"""
    c = RR.case(S)
    dens, z, rays, dgt = (c[k].double() for k in ("dens", "z", "rays", "depth_gt"))
    p = RR.ray_parts(dens, z, rays)
    out = RR.forward(dens, z, rays)
    for k in ("weights", "opacity", "depth", "variance"):
        assert rel(p["w" if k == "weights" else k], out[k]) < 1e-13, k
    for which in RR.COTANGENT_SETS:
        ref = RR.backward_reference(S, which)
        G, gD_tot, _ = RR.kernel_G_render(p, ref["cot"])
        assert rel(G, ref["G"]) < 1e-12
        d_sigma, d_rays = RR.manual_backward(p, G, gD_tot)
        M, D = ref["M"], ref["D"]
        assert float(((d_sigma - ref["g64"][0]).abs() - 1e-12 * M).max()) <= 0
        assert float(((d_rays[:, 3:6] - ref["g64"][1][:, 3:6]).abs().max(1).values - 1e-12 * D).max()) <= 0
        assert float(((d_rays[:, 12] - ref["g64"][1][:, 12]).abs() - 1e-12 * ref["far_mag"]).max()) <= 1e-300
        assert float((ref["g64"][0].abs() - M * (1 + 1e-9)).max()) <= 0
    for sel in RR.SELECTIONS:
        ref = RR.loss_reference(S, sel)
        pc = ref["pieces"]
        assert rel(pc["G"], ref["G"]) < 1e-12 and rel(pc["target"], ref["r64"]["aux"]["target"]) < 1e-13
        for k, t in zip(("depth", "los", "opacity"), ref["r64"]["terms"]):
            assert abs(float(pc["terms"][k].sum()) - float(t)) <= 1e-12 * abs(float(t)) + 1e-300, (sel, k)
        d_sigma, d_rays = RR.manual_backward(p, pc["G"], pc["gD"])
        assert float(((d_sigma - ref["r64"]["d_sigma"]).abs() - 1e-12 * ref["M"]).max()) <= 0
        assert float(((d_rays[:, 3:6] - ref["r64"]["d_rays"][:, 3:6]).abs().max(1).values - 1e-12 * ref["D"]).max()) <= 0
        assert float(((d_rays[:, 12] - ref["r64"]["d_rays"][:, 12]).abs() - 1e-12 * ref["far_mag"]).max()) <= 1e-300
        assert float((ref["r64"]["d_sigma"].abs() - ref["M"] * (1 + 1e-9)).max()) <= 0
        # the kept-ray form of the terms with every ray kept is the oracle's own result
        keep = torch.ones(RR.N_RAYS, dtype=torch.bool)
        t5 = RR.loss_terms(S, sel, keep, F64)
        assert abs(float(t5[0]) - float(ref["r64"]["loss"])) <= 1e-13 * abs(float(ref["r64"]["loss"]))
        assert abs(float(t5[4]) / RR.N_RAYS - float(ref["r64"]["aux"]["depth_eps"])) <= 1e-13 * float(t5[4])
        # and with rays left out it is the sum of the kept rays' own terms under the whole batch's normalisers
        keep[[0, 5, 7, 20]] = False
        t5 = RR.loss_terms(S, sel, keep, F64)
        for k, name in ((0, "total"), (1, "depth"), (2, "los"), (3, "opacity")):
            want = float(pc["terms"][name][keep].sum())
            assert abs(float(t5[k]) - want) <= 1e-12 * abs(want) + 1e-300, (sel, name)
        assert abs(float(t5[4]) - float(ref["eps64"][keep].sum())) <= 1e-13 * float(t5[4])


# ------------------------------------------------------------------------------------------- truth against finite differences
def _central4(f, h):
    """fourth-order central difference of f at 0"""
    return (8.0 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12.0 * h)


@pytest.mark.parametrize("S", [7, 100])
@pytest.mark.parametrize("scalar", ["L2_JS frozen eps", "render_backward"])
def test_float64_autograd_agrees_with_central_differences(S, scalar):
    """d_sigma at 12 samples and the four ray columns at 3 rays, to 1e-6 of the term magnitude.  The samples are drawn among those
    with a density above 0.1 (the stencil stays on one side of relu) and a magnitude within 1e3 of the case's largest (the
    difference quotient's own rounding is 1e-13 of the scalar); the rays for the direction columns likewise, and the far column
    is taken at the three rays where its term is largest."""
    c = RR.case(S)
    dens, z, rays, dgt = (c[k].double() for k in ("dens", "z", "rays", "depth_gt"))
    if scalar == "render_backward":
        ref = RR.backward_reference(S, "all")
        value = lambda d, r: RR.render_scalar(RR.forward(d, z, r), ref["cot"])
        d_sigma, d_rays = ref["g64"]
    else:
        full = RR.loss_reference(S, "L2_JS")
        eps = full["eps64"][:, None]
        value = lambda d, r: RR._lidar_loss(RR.forward(d, z, r), z, r, dgt, "L2_JS", eps_frozen=eps)[0]
        frozen = RR.loss_run(dens, z, rays, dgt, "L2_JS", eps_frozen=eps)
        ref = full
        d_sigma, d_rays = frozen["d_sigma"], frozen["d_rays"]
        assert torch.equal(d_sigma, full["r64"]["d_sigma"]) and torch.equal(d_rays, full["r64"]["d_rays"])   # eps carries no gradient
    M, D, far_mag = ref["M"], ref["D"], ref["far_mag"]
    cand = torch.nonzero((dens > 0.1) & (M > 1e-3 * M.max()))
    gen = torch.Generator().manual_seed(S)
    picks = cand[torch.randperm(cand.shape[0], generator=gen)[:12]]
    assert picks.shape[0] == 12
    for i, k in picks.tolist():
        def f(h):
            d = dens.clone()
            d[i, k] += h
            return float(value(d, rays))
        fd = _central4(f, 0.02)
        assert abs(fd - float(d_sigma[i, k])) <= 1e-6 * float(M[i, k]), (i, k, fd, float(d_sigma[i, k]), float(M[i, k]))
    dir_rays = torch.nonzero(D > 1e-3 * D.max())[:, 0]
    dir_rays = dir_rays[torch.randperm(dir_rays.shape[0], generator=gen)[:3]].tolist()
    far_rays = torch.argsort(far_mag, descending=True)[:3].tolist()                # the three rays with the largest far term
    assert len(dir_rays) == 3 and float(far_mag[far_rays[-1]]) > 0
    for i, col in [(i, col) for i in dir_rays for col in (3, 4, 5)] + [(i, 12) for i in far_rays]:
        def f(h):
            r = rays.clone()
            r[i, col] += h
            return float(value(dens, r))
        fd = _central4(f, 1e-3)
        mag = float(D[i]) if col < 6 else float(far_mag[i])
        assert abs(fd - float(d_rays[i, col])) <= 1e-6 * mag, (i, col, fd, float(d_rays[i, col]), mag)


# ------------------------------------------------------------------------------------------- truth against the recorded reference
def test_float64_restatement_reproduces_golden_g5_render():
    g = {k: torch.from_numpy(v) for k, v in load_golden("g5_render").items()}
    n, S = g["z"].shape
    rays = torch.zeros(n, 13)
    rays[:, 3:6], rays[:, 12] = g["dirs"], g["far"][:, 0]
    dens = (g["sigma"] + g["noise"]).double()
    out = RR.forward(dens, g["z"].double(), rays.double())
    assert rel(out["depth"], g["depth"]) < 1e-5 and rel(out["weights"], g["weights"]) < 1e-5
    assert rel(out["opacity"], g["opacity"]) < 1e-5 and rel(out["variance"], g["variance"]) < 1e-4
    cot = dict(depth=g["cot_depth"], weights=g["cot_weights"], opacity=g["cot_opacity"], variance=g["cot_variance"])
    d_sigma, d_rays = RR.render_grads(dens, g["z"].double(), rays.double(), cot)
    assert rel(d_sigma, g["dsigma"]) < 1e-4
    assert rel(d_rays[:, 3:6], g["ddirs"]) < 1e-4 and rel(d_rays[:, 12], g["dfar"][:, 0]) < 1e-4


def test_float64_restatement_reproduces_golden_g8_compute_loss():
    """the density comes from the oracle network in float32 (as the kernel test takes it from the density kernel); everything behind
    it is the float64 restatement, whose d_sigma is carried on to the parameters and the ray records by the network's autograd"""
    g = load_golden("g8_compute_loss")
    enc = {k: (int(v) if v.isdigit() else v) for k, v in zip(g["enc_keys"], g["enc_vals"])}
    spec = NW.NetworkSpec.from_config(enc, dict(activation="ReLU", n_neurons=32, n_hidden_layers=1))
    rays, z, depths = torch.from_numpy(g["rays"]), torch.from_numpy(g["z"]), torch.from_numpy(g["depths"])
    params = torch.from_numpy(g["params"]).clone().requires_grad_(True)
    rays_leaf = rays.clone().requires_grad_(True)
    sigma = NW.density(spec, params, ORD.sample_points(rays_leaf, z).reshape(-1, 3)).reshape(z.shape)
    dens = (sigma.detach() + torch.from_numpy(g["noise"])).double()
    scale = float(g["scale"].reshape(-1)[0])
    r = RR.loss_run(dens, z.double(), rays.double(), depths.double(), "L1_JS", scale=scale)
    assert rel(r["out"]["weights"], g["weights"]) < 1e-4 and rel(r["out"]["depth"], g["depth"]) < 1e-4
    assert rel(r["out"]["opacity"], g["opacity"]) < 1e-4 and rel(r["out"]["variance"], g["variance"]) < 1e-3
    assert abs(float(r["loss"]) - float(g["loss"])) / float(g["loss"]) < 1e-4
    assert abs(float(r["aux"]["depth_eps"]) - float(g["depth_eps"])) < 1e-4
    sigma.backward(r["d_sigma"].float())
    assert rel(params.grad, g["dparams"]) < 2e-4
    assert rel(rays_leaf.grad.double() + r["d_rays"], g["drays"]) < 2e-4


# ------------------------------------------------------------------------------------------- the cases keep their conditions
def _rows_have_a_bound(x32, x64, mag):
    noise, mag = RR.row_blocks(x32, x64, mag)
    assert bool(((RR.limit(noise, mag) > 0) | (x64.abs().reshape(RR.N_RAYS, -1).max(1).values == 0)).all())


def _case_has_a_bound(x32, x64, mag):
    assert RR.limit(RR.block_err(x32, x64), max(RR.block_max(x64), mag)) > 0 or RR.block_max(x64) == 0


@pytest.mark.parametrize("S", RR.SAMPLE_COUNTS)
def test_cases_keep_their_conditions(S):
    c = RR.case(S)
    assert all(c[k].dtype == F32 for k in ("sigma", "noise", "dens", "z", "rays", "depth_gt"))
    assert torch.equal(c["dens"], c["sigma"] + c["noise"])
    assert float(c["sigma"].abs().min()) >= 1e-3 and float(c["dens"].abs().min()) >= 1e-3
    assert bool((c["z"][:, 1:] >= c["z"][:, :-1]).all()) and float(c["z"].min()) >= 0.02 and float(c["z"].max()) <= 0.90
    norm = c["rays"][:, 3:6].double().norm(dim=1)
    assert float(norm.min()) >= 0.9 - 1e-6 and float(norm.max()) <= 1.1 + 1e-6
    far0 = float(c["rays"][0, 12])
    dgt = c["depth_gt"]
    opaque = (dgt > 0) & ~(dgt > far0)
    assert int(opaque.sum()) >= 6 and int((dgt > far0).sum()) >= 3 and int((dgt == 0).sum()) >= 3
    assert bool((c["dens"][RR.DENSE] > 0).all()) and bool(opaque[RR.DENSE])       # one ray is dense at every sample
    for sel in RR.SELECTIONS:
        ref = RR.loss_reference(S, sel)
        assert torch.equal(ref["opaque"], opaque) and ref["counts"] == (RR.N_RAYS, int(opaque.sum()))
        assert int((~ref["decided"]).sum()) <= 2, (sel, torch.nonzero(~ref["decided"])[:, 0].tolist())
        js = ref["r64"]["aux"]["js"]
        cfg = RR.loss_config(sel)
        if S >= 63:
            assert int((js < cfg.min_js).sum()) >= 2 and int((js > cfg.max_js).sum()) >= 2
            assert int(((js >= cfg.min_js) & (js <= cfg.max_js)).sum()) >= 2
        # no block's bound is zero while its reference is non-zero
        blocks = [(ref["r32"]["d_sigma"], ref["r64"]["d_sigma"], ref["M"].max(1).values),
                  (ref["r32"]["d_rays"][:, 3:6], ref["r64"]["d_rays"][:, 3:6], ref["D"])]
        for x32, x64, mag in blocks:
            _rows_have_a_bound(x32, x64, mag)
        _case_has_a_bound(ref["r32"]["d_rays"][:, 12], ref["r64"]["d_rays"][:, 12], float(ref["far_mag"].max()))
    for which in RR.COTANGENT_SETS:
        ref = RR.backward_reference(S, which)
        for x32, x64, mag in ((ref["g32"][0], ref["g64"][0], ref["M"].max(1).values), (ref["g32"][1][:, 3:6], ref["g64"][1][:, 3:6], ref["D"])):
            _rows_have_a_bound(x32, x64, mag)
        _case_has_a_bound(ref["g32"][1][:, 12], ref["g64"][1][:, 12], float(ref["far_mag"].max()))
    fwd = RR.forward_reference(S)
    _rows_have_a_bound(fwd["f32"]["weights"], fwd["f64"]["weights"], fwd["weights_mag"])
    leaning = [_leaning_parts(c["dens"], c["z"], c["rays"], lean) for lean in (1.0, -1.0)]
    for key in ("depth", "opacity", "variance"):
        _rows_have_a_bound(fwd["f32"][key], fwd["f64"][key], fwd["mag"][key])
        # float32 against 4 ulp of the ray's magnitude alone (no noise term): the oracle's own run, and one whose exponential leans
        mag = torch.maximum(fwd["mag"][key], fwd["f64"][key].abs())
        for x in [fwd["f32"][key]] + [_leaning_scalar(p, key) for p in leaning]:
            assert float(((x.double() - fwd["f64"][key]).abs() - RR.limit(0.0, mag)).max()) <= 0, key


# ------------------------------------------------------------------------------------------- the yardstick sees the slips
def _misses(check):
    """check(ledger) compares a slipped result; -> whether at least one block missed its bound"""
    led = RR.Ledger()
    check(led)
    return len(led.failures) > 0


def _gradient_checks(led, ref, g32, g64, d_sigma, d_rays):
    RR.check_rows(led, "d_sigma", d_sigma, g32[0], g64[0], ref["M"].max(1).values)
    RR.check_rows(led, "directions", d_rays[:, 3:6], g32[1][:, 3:6], g64[1][:, 3:6], ref["D"])
    RR.check_case(led, "far", d_rays[:, 12], g32[1][:, 12], g64[1][:, 12], float(ref["far_mag"].max()))


@pytest.mark.parametrize("S", SLIP_COUNTS)
def test_the_unslipped_restatement_passes_and_every_slip_misses_a_bound(S):
    C = RR.chunk_for(S)
    c = RR.case(S)
    dens, z, rays, dgt = (c[k].double() for k in ("dens", "z", "rays", "depth_gt"))
    fwd = RR.forward_reference(S)
    p = RR.ray_parts(dens, z, rays)
    back = RR.backward_reference(S, "all")
    G, gD_tot, _ = RR.kernel_G_render(p, back["cot"])

    def render_check(d_sigma, d_rays):
        return lambda led: _gradient_checks(led, back, back["g32"], back["g64"], d_sigma, d_rays)

    def loss_check(ref, d_sigma, d_rays):
        return lambda led: _gradient_checks(led, ref, (ref["r32"]["d_sigma"], ref["r32"]["d_rays"]), (ref["r64"]["d_sigma"], ref["r64"]["d_rays"]),
                                            d_sigma, d_rays)

    weights_check = lambda w: (lambda led: RR.check_rows(led, "weights", w, fwd["f32"]["weights"], fwd["f64"]["weights"], fwd["weights_mag"]))
    # nothing slipped: every block passes
    assert not _misses(weights_check(p["w"]))
    assert not _misses(render_check(*RR.manual_backward(p, G, gD_tot)))
    # (a) the suffix sum includes its own sample
    assert _misses(render_check(*RR.manual_backward(p, G, gD_tot, slip="a")))
    # (b) the gap after a lane's last sample is taken from two samples on
    assert _misses(weights_check(RR.ray_parts(dens, z, rays, gaps=RR.lane_gap_slip(z, C))["w"]))
    # (c) the variance's path through depth is dropped
    for which in ("all", "variance"):
        bk = RR.backward_reference(S, which)
        Gc, gDc, _ = RR.kernel_G_render(p, bk["cot"], slip="c")
        assert _misses(lambda led: _gradient_checks(led, bk, bk["g32"], bk["g64"], *RR.manual_backward(p, Gc, gDc))), which
    # (d) the far column without (1 - opacity)
    assert _misses(render_check(*RR.manual_backward(p, G, gD_tot, slip="d")))
    for sel in RR.SELECTIONS:
        ref = RR.loss_reference(S, sel)
        pc = ref["pieces"]
        assert not _misses(loss_check(ref, *RR.manual_backward(p, pc["G"], pc["gD"]))), sel
        assert _misses(loss_check(ref, *RR.manual_backward(p, pc["G"], pc["gD"], slip="a"))), sel
        assert _misses(loss_check(ref, *RR.manual_backward(p, pc["G"], pc["gD"], slip="d"))), sel
        # (e) the target's normaliser counts the 64 C - S padding slots as samples at depth 0: visible where the shallow ray's window
        # reaches depth 0 - always under the LOS selections, under the JS selections where js gives that ray a margin above its depth
        g_shallow = float(dgt[RR.SHALLOW]) * RR.SCALE
        assert sel.endswith("JS") or float(ref["eps64"][RR.SHALLOW]) > g_shallow + 0.5
        if float(ref["eps64"][RR.SHALLOW]) > g_shallow + 0.5:
            keep = torch.ones(RR.N_RAYS, dtype=torch.bool)
            slipped = RR.loss_pieces(p, dgt, sel, float(ref["far0"]), ref["counts"], ref["eps64"], pad_slots=64 * C - S)
            t32, t64 = RR.loss_terms(S, sel, keep, F32), RR.loss_terms(S, sel, keep, F64)
            los_mag = RR.loss_term_magnitudes(ref, keep)[2]
            los_err = abs(float(slipped["terms"]["los"].sum()) - float(t64[2]))
            assert _misses(lambda led: led.figures("los term", los_err, abs(float(t32[2]) - float(t64[2])), los_mag)), sel


# ------------------------------------------------------------------------------------------- the per-ray statistics
def _leaning_parts(dens, z, rays, lean):
    """ray_parts in float32 with an exponential that errs by `lean` ulp, the same way at every sample of positive density"""
    p = dict(RR.ray_parts(dens, z, rays))
    e = torch.where(p["pos"], (p["e"].double() * (1.0 + lean * RR.F32_EPS)).float(), p["e"])
    tt = 1.0 - (1.0 - e) + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(tt[:, :1]), tt], dim=1), dim=1)[:, :-1]
    w = (1.0 - e) * T
    p.update(e=e, tt=tt, T=T, w=w, opacity=w.sum(1))
    p["depth"] = (w * z).sum(1) + (1.0 - p["opacity"]) * rays[:, 12]
    return p


def _leaning_scalar(p, key):
    if key != "variance":
        return p[key]
    return (p["w"] * (p["depth"][:, None] - p["z"]) ** 2).sum(1)


def test_loss_sample_counts_are_the_counts_the_fused_loss_accepts():
    assert RR.LOSS_SAMPLE_COUNTS == (2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024)
    assert all(RR.chunk_for(S) <= 16 for S in RR.LOSS_SAMPLE_COUNTS) and RR.chunk_for(RR.LOSS_MAX_SAMPLES + 1) == 32


@pytest.mark.parametrize("S", RR.LOSS_SAMPLE_COUNTS)
def test_float64_statistics_are_the_oracles_and_float32_stays_inside_their_magnitudes(S):
    c = RR.case(S)
    for sel in RR.SELECTIONS:
        ref = RR.loss_reference(S, sel)
        st, keep = ref["stats"], ref["decided"]
        assert int((~keep).sum()) <= 2                                              # the cap the GPU test relies on
        oracle = RR.oracle_statistics(ref["r64"], RR.N_RAYS)
        assert st["f64"].dtype == F64 and st["f32"].dtype == F32 and bool(torch.isfinite(st["mag"]).all())
        for k, name in enumerate(RR.STAT_NAMES):
            assert float(((st["f64"][:, k] - oracle[:, k]).abs() - 1e-12 * st["mag"][:, k]).max()) <= 0, (sel, name)
        if sel.endswith("LOS"):                                                      # js selects nothing: the configured number, bit for bit
            assert torch.equal(st["f32"][:, 3], torch.full((RR.N_RAYS,), RR.FIXED_EPS)) and torch.equal(st["f64"][:, 3], st["f32"][:, 3].double())
        # float32 against 4 ulp of the magnitude alone (no noise term): the oracle's own run, the restatement's, and one whose exp leans
        runs = [("oracle", st["f32"]), ("restatement", RR.ray_statistics(RR.ray_parts(c["dens"], c["z"], c["rays"]), c["depth_gt"], sel))]
        runs += [(f"lean {lean:+g}", RR.ray_statistics(_leaning_parts(c["dens"], c["z"], c["rays"], lean), c["depth_gt"], sel)) for lean in (1.0, -1.0)]
        for what, x in runs:
            for k, name in enumerate(RR.STAT_NAMES):
                mag = torch.maximum(st["mag"][:, k], st["f64"][:, k].abs())
                over = (x[:, k].double() - st["f64"][:, k]).abs() - RR.limit(0.0, mag)
                assert float(over[keep].max()) <= 0, (sel, what, name, int(over[keep].argmax()))


@pytest.mark.parametrize("S", LOSS_SLIP_COUNTS)
def test_statistics_slips_miss_a_bound_at_every_tier(S):
    c = RR.case(S)
    for sel in RR.SELECTIONS:
        ref = RR.loss_reference(S, sel)
        keep, p = ref["decided"], ref["parts"]
        dgt = c["depth_gt"].double()
        missed = lambda x: {name for name in RR.STAT_NAMES if _misses(lambda led: RR.check_statistics(led, x[keep][:, [RR.STAT_NAMES.index(name)] * 4], _only(ref, name), keep))}
        assert missed(RR.ray_statistics(RR.ray_parts(c["dens"], c["z"], c["rays"]), c["depth_gt"], sel).double()) == set(), sel
        assert missed(RR.ray_statistics(p, dgt, sel)) == set(), sel
        assert {"sd", "js"} <= missed(RR.ray_statistics(p, dgt, sel, slip="f")), sel      # (f) the variance about the rendered depth
        assert {"sd", "js"} <= missed(RR.ray_statistics(p, dgt, sel, slip="g")), sel      # (g) the variance not divided by wden
        slipped = missed(RR.ray_statistics(p, dgt, sel, slip="h"))                        # (h) js below min_js not zeroed
        assert slipped == ({"eps"} if sel.endswith("JS") else set()), sel


def _only(ref, name):
    """the reference with every statistics column replaced by `name`'s (check_statistics then judges that column four times)"""
    k = RR.STAT_NAMES.index(name)
    return dict(stats={key: v[:, [k] * 4] for key, v in ref["stats"].items()})
