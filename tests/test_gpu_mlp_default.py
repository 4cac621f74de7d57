"""The MLP kernels of the default shape class ALONE - routes bf3 (mlp_forward / backward_bf3_kernel), fast32 (mlp_forward / backward_
relu32_kernel) and f16_fast (mlp_forward / backward_f16_kernel), 16 / 32 / 64 neurons - against tests/mlp_restatement.py; needs an MI355X.

The encoder is the known quantity here (tests/test_gpu_encode.py measures it with the MLP as a selector): what is compared is the
arithmetic of the MLP kernels over a persistent loop of three steps, a ragged last tile, the wave-uniform skip path and the slab fold.

Sizes.  n = 2 R + 5 tile + 17 with R = grid x 4 waves x tile from the route the library reports at that size (lnr_density_route): every
wave runs two steps, six or seven run a third, the last tile is partly filled and its last pair half filled.  If the workgroup caps
change, the assertions of `_shape` fail instead of the coverage silently shrinking to one step.

Part A - exact.  On the dyadic lattices of mlp_restatement every product and every partial sum in any order is a float32 (fp16 route:
fp16) number, so sigma, dW1 and dWo have one correct bit pattern and all three routes must return it (tests/test_mlp_host.py recomputes
the preconditions of every case).  ReLU ties (Z == 0 exactly on 0.05 - 1.6 % of the units) are part of it: `Z > 0` must agree.
The backward's d_sigma is live on about 1/8 of the samples and exactly 0 on a stretch 3 tiles + 6 samples longer than a round, so every
wave meets the skip path, the first waves run live - dead - live and two run dead - dead - live.  (A stretch of two whole rounds, as first
planned, would leave 177 live samples at this size.)  d_feature is seen through the encode backward: table gradient per level and
entry and d_pts per point with the bounds of test_gpu_encode.py, whose reference takes the EXACT float64 d_feature.
Rays form: S = 96 as planned, and S = 93 as well, because a live count times 96 = 3 x 32 can never leave the last 32-sample step ragged.

Part B - random default-class networks against float64 (bf3 and fast32; f16_fast at tolerance stays with test_fp16_mode_config5_
4096x256).  Lattice operands have at most 16 significant bits: their third bf16 term is zero and the products (0,2), (2,0) contribute
nothing, so only random operands see a dropped or mis-paired partial product.  Bounds (tail_restatement.Ledger, none taken from the
kernel): 4 x the error of the restatement's sequential float32 run on the block + 4 ulp of the block's largest reference entry;
blocks: 32 consecutive samples of sigma, a neuron row of dW1, dWo, a level of the table gradient (plus its record budget), and d_pts
with its per-point bound.  Samples with a unit within 2^-20 max|Z| of the ReLU kink get d_sigma = 0 and are left out of the sigma blocks.
"""
import functools

import numpy as np
import pytest
import torch

from tests import encode_restatement as ER
from tests import mlp_restatement as MR
from tests.test_gpu_kernels import NETS

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
ROUTE_H = [(route, H) for route in MR.ROUTES for H in MR.WIDTHS]
POISON = -12345.0
DEFAULT_CLASS = {64: "default", 32: "default_n32", 16: "default_n16"}
TABLE_GAIN = 3000.0
KINK = 2.0 ** -20


def dv(x, dtype=torch.float32):
    return x.to(DEV, dtype).contiguous()


@pytest.fixture(scope="module")
def ops():
    from loner_amd import ops as _ops
    from loner_amd import hip
    hip.load()
    return _ops


def _spec(route, H, enc=None):
    from loner_amd import hip
    spec = hip.make_net_spec(MR.LATTICE_ENC if enc is None else enc, MR.net_config(route, H))
    if enc is None:
        assert [float(spec.level_scale[l]) for l in range(16)] == [float(2 ** (l + 1) - 1) for l in range(16)]
    return spec


def _shape(route, H, backward, enc=None):
    """MR.launch (which asserts the route) + what the size is chosen for"""
    s = MR.launch(route, H, backward, enc)
    assert MR.waves_with_three_steps(s) >= 1 and s["n"] % s["tile"] != 0 and s["n"] % 2 == 1 and s["n"] > 2 * s["R"]
    return s


def _same_route(route, H, backward, n, shape=None, enc=None):
    """the route at another size (with `shape`: and its launch shape) is the one under test"""
    from tests.support import density_route
    got = density_route(MR.LATTICE_ENC if enc is None else enc, MR.net_config(route, H), n, backward, shape=True)
    assert got["route"] == route and (shape is None or (got["grid"], got["tile"]) == (shape["grid"], shape["tile"])), got


def _assert_bits(what, got, ref, shape=None):
    """torch.equal with a report of the first difference; shape: the entries are samples of that launch"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = torch.nonzero((got != ref).reshape(-1))[:, 0]
    i = int(bad[0])
    where = f"sample {i} {MR.coordinates(i, shape)}" if shape is not None else f"entry {tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))}"
    pytest.fail(f"{what}: {bad.numel()} of {ref.numel()} entries differ; first: {where}: kernel {float(got.reshape(-1)[i])!r} "
                f"reference {float(ref.reshape(-1)[i])!r}; last: entry {int(bad[-1])}")


def _finish(ledger):
    failures = ledger.report()
    assert not failures, "\n".join(failures)


# =========================================================================================== Part A: exact
@pytest.mark.parametrize("route,H", ROUTE_H)
def test_forward_is_bit_exact_on_the_lattice(ops, route, H):
    s = _shape(route, H, False)
    c = MR.forward_case(MR.FORWARD_LATTICE[route]["name"], s["n"], H)
    sigma = ops.density_forward(_spec(route, H), dv(c["params"]), pts=dv(c["pts"]))
    _assert_bits(f"sigma {route} H={H}", sigma, c["sigma64"].float(), s)


@functools.lru_cache(maxsize=None)
def _encode_reference(n, tile, R, H):
    """(float32 run, float64 run, per-point magnitude) of the encode backward on the exact float64 d_feature of a backward case"""
    c = MR.backward_case(n, tile, R, H)
    d_feat, live = c["r64"]["d_feature"], c["d_sigma"] != 0          # (1/15 of the samples are live: the others contribute exact zeros)
    r32 = ER.encode_gradients_of_live(c["grid"], c["table"], c["pts"], F32, d_feat.float(), live)
    r64 = ER.encode_gradients_of_live(c["grid"], c["table"], c["pts"], F64, d_feat, live)
    return r32, r64, ER.input_magnitude_of_live(c["grid"], c["table"], c["pts"], d_feat, live)


@pytest.mark.parametrize("route,H", ROUTE_H)
def test_backward_is_bit_exact_on_the_lattice(ops, route, H):
    s = _shape(route, H, True)
    n = s["n"]
    c = MR.backward_case(n, s["tile"], s["R"], H)
    lo, hi = c["dead"]
    # the conditions of the case (tests/test_mlp_host.py has them too): the stretch is longer than a round, every step outside it holds a
    # live sample, every step inside it is skipped, and the live steps hold pairs with both, only the even and only the odd sample live
    dead = MR.dead_tiles(c["d_sigma"], s["tile"])
    inside = torch.zeros(dead.numel(), dtype=torch.bool)
    inside[(lo + s["tile"] - 1) // s["tile"]:hi // s["tile"]] = True
    assert hi - lo > s["R"] and torch.equal(dead, inside) and min(MR.pair_kinds(c["d_sigma"])) > 0
    spec, params, pts, ds = _spec(route, H), dv(c["params"]), dv(c["pts"]), dv(c["d_sigma"])
    n_mlp = int(spec.n_mlp_params)
    # every d_feature row holds something before the call under test: a skipped step must still write its zeros
    ops.density_backward(spec, params, torch.ones(n, device=DEV), torch.zeros(int(spec.n_params), device=DEV), pts=pts, want_d_pts=True)
    grad = torch.zeros(int(spec.n_params), device=DEV)
    d_pts = ops.density_backward(spec, params, ds, grad, pts=pts, want_d_pts=True)
    gW1, gWout = MR.unpack(grad.cpu(), H)
    case = f"lattice backward {route} H={H}"
    _assert_bits(f"{case}: dW1", gW1, c["r64"]["dW1"].float())
    _assert_bits(f"{case}: dWo", gWout[0], c["r64"]["dWo"].float())
    assert not bool(gWout[1:].any()), "output rows 1..15 received a gradient"
    stale = torch.nonzero(d_pts[lo:hi].cpu().abs().sum(dim=1))[:, 0]
    assert stale.numel() == 0, f"d_pts is not zero on {stale.numel()} samples of the dead stretch; first: {MR.coordinates(lo + int(stale[0]), s)}"
    r32, r64, mag = _encode_reference(n, s["tile"], s["R"], H)
    led = ER.EncodeLedger()
    ER.check_table(led, case, c["grid"], grad, r32, r64)
    ER.check_points(led, case, d_pts, r32, r64, mag)
    # without the input gradient: the same weight and table gradients
    grad2 = torch.zeros_like(grad)
    assert ops.density_backward(spec, params, ds, grad2, pts=pts) is None
    _assert_bits(f"{case}: MLP gradient without d_pts", grad2[:n_mlp], grad[:n_mlp])
    assert torch.equal(grad2[n_mlp:], grad[n_mlp:]), "table gradient differs without d_pts"
    # the slab fold on its own
    grad3 = torch.zeros_like(grad)
    ops.density_backward(spec, params, ds, grad3, pts=pts, want_d_pts=True, defer_weight_fold=True)
    assert not bool(grad3[:n_mlp].any()), "a deferred fold wrote weight gradients"
    ops.density_fold_weight_grads(spec, grad3, n)
    _assert_bits(f"{case}: MLP gradient with the deferred fold", grad3[:n_mlp], grad[:n_mlp])
    _finish(led)


@functools.lru_cache(maxsize=None)
def _rays_sigma(n, S, H):
    c, inp = MR.rays_case(n, S), MR.lattice_inputs("coarse", n, H)
    feat = MR.lattice_features(inp["grid"], inp["table"], c["pts"][:c["M"]], F64)
    return MR.mlp(feat, inp["W1"].double(), inp["wo"].double())[0].float()


@pytest.mark.parametrize("S", MR.RAY_SAMPLES)
@pytest.mark.parametrize("route,H", ROUTE_H)
def test_rays_form_with_a_device_side_live_count(ops, route, H, S):
    s = _shape(route, H, True)
    c, inp = MR.rays_case(s["n"], S), MR.lattice_inputs("coarse", s["n"], H)
    M, live, n_rays = c["M"], c["live"], c["n_rays"]
    assert live < n_rays and M > 2 * s["R"] + s["tile"] and (M % 32 != 0) == (S % 32 != 0)
    _same_route(route, H, False, n_rays * S)
    _same_route(route, H, True, n_rays * S, s)
    spec, params = _spec(route, H), dv(inp["params"])
    n_mlp = int(spec.n_mlp_params)
    rays, z, n_dev = dv(c["rays"]), dv(c["z"]), torch.tensor([live], dtype=torch.int32, device=DEV)
    out = torch.full((n_rays, S), POISON, device=DEV)
    assert ops.density_forward(spec, params, rays=rays, z=z, n_rays_dev=n_dev, out=out) is out
    flat = out.reshape(-1).cpu()
    shape_m = dict(s, n=M)
    _assert_bits(f"rays S={S} {route} H={H}: sigma of the live rays", flat[:M], _rays_sigma(s["n"], S, H), shape_m)
    assert bool((flat[M:] == POISON).all()), f"sigma written beyond the live rays: first at sample {M + int(torch.nonzero(flat[M:] != POISON)[0, 0])}"
    d_sigma = MR.lattice_d_sigma(n_rays * S, MR.D_SIGMA_SEED + S)
    assert bool(d_sigma[M:].any())                                  # the dead rays carry a gradient that must be ignored
    grad_r = torch.zeros(int(spec.n_params), device=DEV)
    ops.density_backward(spec, params, dv(d_sigma.reshape(n_rays, S)), grad_r, rays=rays, z=z, n_rays_dev=n_dev)
    grad_p = torch.zeros_like(grad_r)
    ops.density_backward(spec, params, dv(d_sigma[:M]), grad_p, pts=dv(c["pts"][:M]))
    assert bool(grad_p[:n_mlp].any())
    _assert_bits(f"rays S={S} {route} H={H}: MLP gradient against the points form", grad_r[:n_mlp], grad_p[:n_mlp])


# =========================================================================================== Part B: random weights against float64
@functools.lru_cache(maxsize=None)
def _random_case(H, n, tile, R):
    """-> dict of a random default-class network at n points: params, pts, d_sigma (kink samples and the dead stretch zeroed), kept (mask
    of the samples away from a kink), the MLP runs m32 / m64 and the encode-backward runs r32 / r64 with the per-point magnitude"""
    from loner_amd import hip
    from oracle import network as NW
    enc = NETS[DEFAULT_CLASS[H]][0]
    spec_o = NW.NetworkSpec.from_config(enc, dict(activation="ReLU", n_neurons=H, n_hidden_layers=1))
    spec_h = hip.make_net_spec(enc, MR.net_config("bf3", H))
    grid = ER.make_grid(enc)
    for l, lv in enumerate(grid.levels):          # the library's own float32 scale defines the cell (tests/test_gpu_encode.py _grid_table)
        assert (lv.res, lv.size, lv.offset, int(lv.hashed)) == (spec_h.level_res[l], spec_h.level_size[l], spec_h.level_offset[l], spec_h.level_hashed[l])
        assert abs(lv.scale - spec_h.level_scale[l]) <= 2e-7 * lv.scale
        lv.scale = float(spec_h.level_scale[l])
    params = NW.init_params(spec_o, seed=40 + H)
    params[spec_o.n_mlp_params:] *= TABLE_GAIN
    table = params[spec_o.n_mlp_params:]
    W1, Wout = MR.unpack(params, H)
    wo = Wout[0].clone()
    gen = torch.Generator().manual_seed(50 + H)
    pts = torch.rand(n, 3, generator=gen) * 1.9 - 0.95
    d_sigma = torch.randn(n, generator=gen) * torch.exp2(-14.0 * torch.rand(n, generator=gen))
    d_sigma[torch.rand(n, generator=gen) < 0.1] = 0.0
    lo, hi = MR.dead_stretch(dict(tile=tile, R=R))
    d_sigma[lo:hi] = 0.0
    f64 = torch.cat(ER.encode(grid, table, pts, F64)["feat"], dim=1)
    Z = MR.preactivations(f64, W1.double())
    kept = ~(Z.abs() < KINK * float(Z.abs().max())).any(dim=1)
    d_sigma = d_sigma * kept
    m64 = MR.backward(f64, W1.double(), wo.double(), d_sigma.double())
    f32 = torch.cat(ER.encode(grid, table, pts, F32)["feat"], dim=1)
    m32 = MR.backward(f32, W1, wo, d_sigma)
    live = d_sigma != 0
    r64 = ER.encode_gradients_of_live(grid, table, pts, F64, m64["d_feature"], live)
    r32 = ER.encode_gradients_of_live(grid, table, pts, F32, m32["d_feature"], live)
    mag = ER.input_magnitude_of_live(grid, table, pts, m64["d_feature"], live)
    keep = ("sigma", "dW1", "dWo", "A_sigma", "A_dW1", "A_dWo")
    return dict(enc=enc, grid=grid, params=params, pts=pts, d_sigma=d_sigma, kept=kept, dead=(lo, hi), mag=mag, r32=r32, r64=r64,
                m32={k: m32[k] for k in keep}, m64={k: m64[k] for k in keep})


@pytest.mark.parametrize("H", MR.WIDTHS)
@pytest.mark.parametrize("route", ["bf3", "fast32"])
def test_random_network_against_float64(ops, route, H):
    enc = NETS[DEFAULT_CLASS[H]][0]
    s = _shape(route, H, True, enc)
    n = s["n"]
    _same_route(route, H, False, n, enc=enc)
    c = _random_case(H, n, s["tile"], s["R"])
    kept, (lo, hi) = c["kept"], c["dead"]
    excluded = 1.0 - float(kept.double().mean())
    print(f"FIGURES random {route} H={H}: n = {n}, {int((~kept).sum())} samples ({excluded:.2e}) within 2^-20 max|Z| of a kink; "
          f"{int((c['d_sigma'] != 0).sum())} live samples")
    assert excluded <= 0.01
    spec, params, pts = _spec(route, H, enc), dv(c["params"]), dv(c["pts"])
    sigma = ops.density_forward(spec, params, pts=pts).cpu().double()
    grad = torch.zeros(int(spec.n_params), device=DEV)
    d_pts = ops.density_backward(spec, params, dv(c["d_sigma"]), grad, pts=pts, want_d_pts=True)
    gW1, gWout = MR.unpack(grad.cpu(), H)
    m32, m64 = c["m32"], c["m64"]
    case = f"random {route} H={H}"
    led = ER.EncodeLedger()
    # sigma: blocks of 32 consecutive samples, the kink samples left out
    pad = (n + 31) // 32 * 32
    def blocks(x):
        out = torch.zeros(pad, dtype=F64)
        out[:n] = x.double() * kept
        return out.reshape(-1, 32)
    err, noise, ref = (blocks(sigma) - blocks(m64["sigma"])).abs().amax(dim=1), (blocks(m32["sigma"]) - blocks(m64["sigma"])).abs().amax(dim=1), \
        blocks(m64["sigma"]).abs().amax(dim=1)
    for b in range(pad // 32):
        led.figures(f"{case}: sigma, 32 samples", float(err[b]), float(noise[b]), float(ref[b]), f"samples {32 * b}.. {MR.coordinates(32 * b, s)}")
    for j in range(H):
        led.block(f"{case}: dW1, neuron row", gW1[j], m32["dW1"][j], m64["dW1"][j], f"neuron {j}")
    led.block(f"{case}: dWo", gWout[0], m32["dWo"], m64["dWo"])
    assert not bool(gWout[1:].any()), "output rows 1..15 received a gradient"
    # the same figures in units of the term sums: error / (2^-23 A), worst entry
    for name, got, key in (("sigma", sigma * kept, "sigma"), ("dW1", gW1, "dW1"), ("dWo", gWout[0], "dWo")):
        A = m64["A_" + key]
        dev = (got.double() - m64[key] * (kept if name == "sigma" else 1.0)).abs()
        d32 = (m32[key].double() - m64[key]).abs() * (kept if name == "sigma" else 1.0)
        ok = A > 0
        print(f"FIGURES {case}: {name} in units of 2^-23 A: kernel {float((dev[ok] / A[ok]).max()) * 2 ** 23:.3f}, cpu float32 {float((d32[ok] / A[ok]).max()) * 2 ** 23:.3f}")
    assert not bool(d_pts[lo:hi].cpu().any()), "d_pts is not zero on the dead stretch"
    # (per level only: an entry sums a few samples' d_feature, and a random network's d_feature is a cancelling sum of H products whose
    # float32 rounding alone exceeds the 2^-17 of the entry limit - both routes and the float32 restatement show it alike)
    ER.check_table(led, case, c["grid"], grad, c["r32"], c["r64"], entries=False)
    ER.check_points(led, case, d_pts, c["r32"], c["r64"], c["mag"])
    _finish(led)
