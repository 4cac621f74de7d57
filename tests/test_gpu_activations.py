"""Every density activation on every MLP route, and the power-of-two scale equivariance of the fp16 backward - needs an MI355X.

Part A: one network per route of the dispatch (tests/support.py ACTIVATION_ROUTES: each case asserts it lands there) x the nine
activations, the hidden weights scaled so that the pre-activations reach each activation's regimes (asserted on the oracle: a case
that stops reaching them fails instead of passing vacuously).  Forward and full backward against oracle/network.py at the same storage
precision, plus a per-sample d_pts check that a global-maximum norm cannot give.

Part B: in the fp16 storage model, multiplying the output row by 2^k multiplies sigma and every gradient but the output row's own by
exactly 2^k as long as every rounded value stays a normal fp16 number: the backward's power-of-two unit must follow the dZ it rounds.
"""
import math

import numpy as np
import pytest
import torch

from oracle import network as NW
from tests.support import ACTIVATION_NAMES, ACTIVATION_ROUTES, density_route, route_of

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dv(x):
    return x.to(DEV, torch.float32).contiguous()


def rel(a, b):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rel_layers(spec_o, grad, ref):
    worst, off = 0.0, 0
    for rows, cols in spec_o.mlp_shapes:
        n = rows * cols
        if float(ref[off:off + n].abs().max()) > 0.0:
            worst = max(worst, rel(grad[off:off + n], ref[off:off + n]))
        off += n
    return worst


@pytest.fixture(scope="module")
def ops():
    from loner_amd import hip
    from loner_amd import ops as _ops
    hip.load()
    return _ops


def _spec(enc, net):
    """oracle and library specs of one network; the oracle takes the library's per-level scales.  With a growth factor that is not a
    power of two the two derive them with different exp2 / log2 evaluations and differ by up to ~2e-7 relative (2.9e-6 at scale 13.9 on the
    18-level x 1.3 grid); on the fine levels that moves every grid position, and sigma, by ~1e-4 - more than the parity tolerances allow,
    and not a property of the MLP routes tested here."""
    from loner_amd import hip
    spec_o, spec_h = NW.NetworkSpec.from_config(enc, net), hip.make_net_spec(enc, net)
    assert spec_o.n_params == int(spec_h.n_params)
    for l, lv in enumerate(spec_o.levels):
        assert abs(lv.scale - spec_h.level_scale[l]) <= 1e-6 * lv.scale
        lv.scale = float(spec_h.level_scale[l])
    return spec_o, spec_h


def _matrices(spec_o, params):
    mats, cur = [], 0
    for o, i in spec_o.mlp_shapes:
        mats.append((cur, o, i))
        cur += o * i
    return mats


def _layer_inputs(spec_o, params, pts):
    """the encoded (padded) input of the first layer, as oracle.network.density_unit forms it"""
    x = (pts + 1) / 2
    if spec_o.enc_type == "HashGrid":
        h = NW.encode_hashgrid(spec_o, params[spec_o.n_mlp_params:].reshape(-1, spec_o.n_features), x)
    else:
        h = NW.encode_frequency(spec_o, x)
    if h.shape[1] < spec_o.in_dim:
        h = torch.cat([h, torch.ones(h.shape[0], spec_o.in_dim - h.shape[1], dtype=h.dtype)], dim=1)
    return h


def _pre_activations(spec_o, params, pts):
    """[pre-activations of every hidden layer] with the oracle's arithmetic (fp16 storage rounding included)"""
    half = spec_o.precision == "fp16"
    h, out = _layer_inputs(spec_o, params, pts), []
    for off, o, i in _matrices(spec_o, params)[:-1]:
        m = params[off:off + o * i].reshape(o, i)
        v = (NW.round_f16(h) if half else h) @ (NW.round_f16(m) if half else m).T
        out.append(v)
        h = NW._activate(v, spec_o.activation)
    return out


K = NW.K_ACT
# how the hidden weights are scaled (layer by layer: ("std", s) = standard deviation s of the pre-activations, ("max", m) = largest |v| m,
# ("std", s, m) = s unless that puts the largest |v| beyond m)
# and the regimes each activation must reach, as predicates on the pre-activations v (>= 5 % of them in each)
REGIMES = {
    "None": (("std", 1.0), {"v < 0": lambda v: v < 0, "v > 0": lambda v: v > 0}),
    "ReLU": (("std", 1.0), {"v < 0": lambda v: v < 0, "v > 0": lambda v: v > 0}),
    "LeakyReLU": (("std", 1.0), {"negative side": lambda v: v < 0, "v > 0": lambda v: v > 0}),
    "Sine": (("std", 3.0), {"|v| < pi/2": lambda v: v.abs() < math.pi / 2, "|v| > pi": lambda v: v.abs() > math.pi}),
    "Exponential": (("std", 1.0, 2.0), {"v < -1/2": lambda v: v < -0.5, "v > 1/2": lambda v: v > 0.5}),
    "Sigmoid": (("std", 6.0), {"|v| < 1": lambda v: v.abs() < 1, "saturated |v| > 5": lambda v: v.abs() > 5}),
    "Tanh": (("std", 4.0), {"|v| < 0.5": lambda v: v.abs() < 0.5, "saturated |v| > 3": lambda v: v.abs() > 3}),
    "Squareplus": (("std", 0.3), {"|K v| < 1": lambda v: (K * v).abs() < 1, "|K v| > 4": lambda v: (K * v).abs() > 4}),
    "Softplus": (("std", 2.5), {"K v <= 20": lambda v: K * v <= 20, "K v > 20": lambda v: K * v > 20}),
}


def _regime_params(spec_o, params, pts):
    """scale the first and hidden matrices, one after the other, so that their pre-activations on `pts` hit the activation's target.
    A hidden matrix first loses the component of its rows along the mean of its inputs: positive activations (Exponential, Sigmoid)
    would otherwise give every neuron a common offset and a single sign."""
    how, target, cap = (REGIMES[spec_o.activation][0] + (math.inf,))[:3]
    p = params.clone()
    for l, (off, o, i) in enumerate(_matrices(spec_o, p)[:-1]):
        if l > 0:
            h = NW._activate(_pre_activations(spec_o, p, pts)[l - 1], spec_o.activation)
            mu = h.mean(dim=0)
            w = p[off:off + o * i].reshape(o, i)
            w -= torch.outer(w @ mu, mu) / float(mu @ mu)
        v = _pre_activations(spec_o, p, pts)[l]
        now = float(v.std()) if how == "std" else float(v.abs().max())
        p[off:off + o * i] *= min(target / now, cap / float(v.abs().max()))
    return p


def _tile_select(d_sigma, tile=32, span=2.0 ** 10):
    """samples whose |d_sigma| is non-zero and within `span` of the largest |d_sigma| of their 32-sample tile"""
    a = d_sigma.abs()
    n = a.shape[0]
    pad = torch.cat([a, torch.zeros((-n) % tile)])
    tmax = pad.reshape(-1, tile).max(dim=1).values.repeat_interleave(tile)[:n]
    return (a > 0) & (a * span >= tmax)


def _per_sample_dpts(d_pts, ref, d_sigma, at_kink=None):
    """largest per-sample d_pts error, each sample against its own oracle magnitude, over the samples of _tile_select (without those
    `at_kink`); the magnitude is floored at 1e-3 of the typical |d_pts| / |d_sigma| times the sample's |d_sigma| (a sample whose three
    components cancel by accident)"""
    sel = _tile_select(d_sigma) if at_kink is None else _tile_select(d_sigma) & ~at_kink
    err = (d_pts.cpu().double() - ref.double()).abs().max(dim=1).values[sel]
    mag = ref.double().abs().max(dim=1).values[sel]
    ds = d_sigma.double().abs()[sel]
    gain = float(torch.median(mag / ds))
    return float((err / torch.maximum(mag, 1e-3 * gain * ds)).max()), int(sel.sum())


# ------------------------------------------------------------------------------------------- A: route x activation
@pytest.mark.parametrize("act", ACTIVATION_NAMES)
@pytest.mark.parametrize("name", list(ACTIVATION_ROUTES))
def test_activation_on_route_matches_oracle(ops, name, act):
    enc, net_base, want = ACTIVATION_ROUTES[name]
    net = dict(net_base, activation=act)
    n = 2000                                                           # ragged: 62.5 tiles of 32, 125 of 16
    expect = dict(want, obj=None) if ("obj" in want and act in ("ReLU", "Sine")) else want
    assert route_of(name, act, n) == expect
    spec_o, spec_h = _spec(enc, net)
    f16 = spec_o.precision == "fp16"
    gen = torch.Generator().manual_seed(7)
    pts = torch.rand(n, 3, generator=gen) * 1.9 - 0.95
    params = NW.init_params(spec_o, 3)
    if spec_o.n_enc_params:
        params[spec_o.n_mlp_params:] *= 3000.0
    params = _regime_params(spec_o, params, pts)
    # the precondition: every layer's pre-activations reach every regime of the activation (Exponential: and stay <= 5)
    for l, v in enumerate(_pre_activations(spec_o, params, pts)):
        for what, pred in REGIMES[act][1].items():
            frac = float(pred(v).double().mean())
            assert frac >= 0.05, f"{name} / {act}: layer {l} has {frac:.1%} of its pre-activations in the regime {what}"
        if act == "Exponential":
            assert float(v.abs().max()) <= 5.0
    d_sigma = torch.randn(n, generator=gen) * torch.exp2(-14 * torch.rand(n, generator=gen))   # magnitudes spread inside every tile
    d_sigma[torch.rand(n, generator=gen) < 0.1] = 0.0

    P, X = dv(params), dv(pts)
    sig = ops.density_forward(spec_h, P, pts=X).cpu()
    grad = torch.zeros(int(spec_h.n_params), device=DEV)
    d_pts = ops.density_backward(spec_h, P, dv(d_sigma), grad, pts=X, want_d_pts=True)
    p32, x32 = params.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    ref = NW.density(spec_o, p32, x32)
    (ref * d_sigma).sum().backward()
    p64, x64 = params.double().requires_grad_(True), pts.double().requires_grad_(True)
    ref64 = NW.density(spec_o, p64, x64)
    (ref64 * d_sigma.double()).sum().backward()

    scale = float(ref.detach().abs().max())
    e_s = float((sig - ref.detach()).abs().max()) / scale
    nm = spec_o.n_mlp_params
    e_p, e_w, e_x = rel(grad, p32.grad), rel(grad[:nm], p32.grad[:nm]), rel(d_pts, x32.grad)
    e_t = rel(grad[nm:], p32.grad[nm:]) if spec_o.n_enc_params else 0.0
    e_l = rel_layers(spec_o, grad, p32.grad)
    # a ReLU / LeakyReLU unit whose pre-activation lies within rounding of the kink may take the other slope in the kernel: a step in that
    # sample's gradient, not an error of it (fp16: the inputs of every layer are rounded to 11 bits)
    at_kink = None
    if act in ("ReLU", "LeakyReLU"):
        eps = 2.0 ** -10 if f16 else 2.0 ** -20
        at_kink = torch.zeros(n, dtype=torch.bool)
        for v in _pre_activations(spec_o, params, pts):
            at_kink |= (v.abs() < eps * v.abs().max()).any(dim=1)
    e_i, n_sel = _per_sample_dpts(d_pts, x32.grad, d_sigma, at_kink)
    print(f"{name} / {act} ({route_of(name, act, n)}): sigma {e_s:.2e}  dparams {e_p:.2e} (dW {e_w:.2e}, dtable {e_t:.2e})  "
          f"dpts {e_x:.2e}  worst matrix {e_l:.2e}  per-sample dpts {e_i:.2e} over {n_sel}  | vs fp64: sigma "
          f"{float((sig.double() - ref64.detach()).abs().max()) / scale:.2e} dparams {rel(grad, p64.grad):.2e} dpts {rel(d_pts, x64.grad):.2e}")
    if f16:
        assert e_s < 2e-3 and e_w < 3e-3 and e_t < 3e-3 and e_x < 5e-3
        assert e_l < 3e-2
        assert e_i < 5e-2
    else:
        assert e_s < 1e-5 and e_p < 2e-5 and e_x < 2e-4
        assert e_l < 2e-4
        assert e_i < 2e-3


# ------------------------------------------------------------------------------------------- B: fp16 scale equivariance
# the three fp16 backward routes, two activations (smooth / kinked), two or three hidden layers
EQUI_NETS = {
    "f16_gen": (dict(otype="HashGrid", n_levels=4, n_features_per_level=2, log2_hashmap_size=12, base_resolution=8),
                dict(n_neurons=64, n_hidden_layers=3, precision="fp16"), "f16_gen"),
    "f16_freq": (dict(otype="Frequency", n_frequencies=8), dict(n_neurons=64, n_hidden_layers=3, precision="fp16"), "f16_freq"),
    "f16_wide": (dict(otype="Frequency", n_frequencies=6), dict(n_neurons=256, n_hidden_layers=2, precision="fp16"), "wide"),
}


def _equi_params(spec_o, seed):
    """initial weights with the output row moved to [2^-8, 0.2] in magnitude: 2^k w is rounded to fp16 exactly as w is, times 2^k, for
    k in [-6, 18]"""
    params = NW.init_params(spec_o, seed)
    if spec_o.n_enc_params:
        params[spec_o.n_mlp_params:] *= 3000.0
    off, o, i = _matrices(spec_o, params)[-1]
    wo = params[off:off + i]                                           # row 0 of the output matrix (rows 1..15 never matter)
    wo.copy_(torch.where(wo.abs() < 2.0 ** -8, torch.where(wo < 0, -(2.0 ** -8), 2.0 ** -8), wo).clamp(-0.2, 0.2))
    return params


def _scaled_output_row(spec_o, params, k):
    off, o, i = _matrices(spec_o, params)[-1]
    p = params.clone()
    p[off:off + i] *= 2.0 ** k
    w, w2 = params[off:off + i], p[off:off + i]
    assert torch.equal(w2.half().float(), w.half().float() * 2.0 ** k), k            # the storage precondition, checked on the CPU
    assert bool(torch.isfinite(w2.half().float()).all()) and float(w2.half().float().abs().min()) >= 2.0 ** -14
    return p


def _run(ops, spec_h, params, d_sigma, pts=None, rays=None, z=None):
    P = dv(params)
    grad = torch.zeros(int(spec_h.n_params), device=DEV)
    if pts is not None:
        sig = ops.density_forward(spec_h, P, pts=dv(pts))
        d_in = ops.density_backward(spec_h, P, dv(d_sigma), grad, pts=dv(pts), want_d_pts=True)
    else:
        R, Z = dv(rays), dv(z)
        sig = ops.density_forward(spec_h, P, rays=R, z=Z)
        d_in = torch.zeros(rays.shape[0], 13, device=DEV)
        ops.density_backward(spec_h, P, dv(d_sigma), grad, rays=R, z=Z, d_rays=d_in)
    torch.cuda.synchronize()
    return sig.cpu(), grad.cpu(), d_in.cpu()


def _assert_equivariant(spec_o, base, run, k, what):
    """run = base with the output row x 2^k: sigma, d_in and every gradient but the output row's x 2^k, bit for bit; the table gradient
    (64-bit fixed-point reduction) per level at 1e-6.  sigma beyond the fp16 range is the reference's clip to +-65504 (fp16 network output,
    finite_or_clipped in lnr_density_impl.h)"""
    f = 2.0 ** k
    sig0, g0, d0 = base
    sig, g, d = run
    bad = []
    want = torch.where((sig0 * f).abs() <= 65504.0, sig0 * f, torch.copysign(torch.full_like(sig0, 65504.0), sig0))
    if not torch.equal(sig, want):
        bad.append(f"sigma (max rel {rel(sig, want):.1e})")
    mats = _matrices(spec_o, g0)
    for l, (off, o, i) in enumerate(mats):
        a, b = g[off:off + o * i], g0[off:off + o * i]
        want = b if l == len(mats) - 1 else b * f
        if not torch.equal(a, want):
            nonfin = int((~torch.isfinite(a)).sum())
            bad.append(f"matrix {l} (max rel {rel(a, want):.1e}, {nonfin} non-finite)")
    for lv in spec_o.levels:
        lo = spec_o.n_mlp_params + lv.offset * spec_o.n_features
        a, b = g[lo:lo + lv.size * spec_o.n_features], g0[lo:lo + lv.size * spec_o.n_features] * f
        if float(b.abs().max()) > 0 and not rel(a, b) < 1e-6:
            bad.append(f"table level {lv} (max rel {rel(a, b):.1e})")
    if not torch.equal(d, d0 * f):
        bad.append(f"input gradient (max rel {rel(d, d0 * f):.1e}, {int((~torch.isfinite(d)).sum())} non-finite)")
    assert not bad, f"{what}, k = {k}: " + "; ".join(bad)


@pytest.mark.parametrize("act", ["Tanh", "ReLU"])
@pytest.mark.parametrize("name", list(EQUI_NETS))
def test_fp16_backward_is_equivariant_under_output_row_scaling(ops, name, act):
    enc, net_base, route = EQUI_NETS[name]
    net = dict(net_base, activation=act)
    assert density_route(enc, net, 1500)["route"] == route
    spec_o, spec_h = _spec(enc, net)
    params = _equi_params(spec_o, 5)
    gen = torch.Generator().manual_seed(9)
    n = 1500
    pts = torch.rand(n, 3, generator=gen) * 1.9 - 0.95
    d_sigma = torch.randn(n, generator=gen)
    base = _run(ops, spec_h, params, d_sigma, pts=pts)
    assert all(bool(torch.isfinite(t).all()) for t in base)
    for k in (-6, 8, 16, 18):
        _assert_equivariant(spec_o, base, _run(ops, spec_h, _scaled_output_row(spec_o, params, k), d_sigma, pts=pts), k, f"{name} / {act}")


@pytest.mark.parametrize("name", list(EQUI_NETS))
def test_fp16_backward_keeps_small_columns_of_a_tile(ops, name):
    """d_sigma spread over 2^-12 .. 1 inside every tile, the output row x 2^-6: the small columns' dZ must stay normal fp16 numbers"""
    enc, net_base, route = EQUI_NETS[name]
    net = dict(net_base, activation="Tanh")
    spec_o, spec_h = _spec(enc, net)
    params = _equi_params(spec_o, 6)
    gen = torch.Generator().manual_seed(10)
    n = 1500
    pts = torch.rand(n, 3, generator=gen) * 1.9 - 0.95
    d_sigma = torch.sign(torch.randn(n, generator=gen)) * torch.exp2(-torch.randint(0, 13, (n,), generator=gen).float())
    base = _run(ops, spec_h, params, d_sigma, pts=pts)
    _assert_equivariant(spec_o, base, _run(ops, spec_h, _scaled_output_row(spec_o, params, -6), d_sigma, pts=pts), -6, f"{name} mixed tile")


@pytest.mark.parametrize("name", ["f16_freq", "f16_wide"])
def test_fp16_backward_scales_each_ray_on_its_own(ops, name):
    """Rays form, 256 samples per ray (every 32-sample tile and every 128-sample step inside one ray): every other ray's d_sigma x 2^-30
    scales that ray's d_rays by exactly 2^-30 and leaves the others'.  (Frequency encodings: their d_rays is an fp32 reduction of d_pts;
    the hash-grid route sums rays in 64-bit fixed point.)"""
    enc, net_base, route = EQUI_NETS[name]
    net = dict(net_base, activation="Tanh")
    spec_o, spec_h = _spec(enc, net)
    params = _equi_params(spec_o, 7)
    gen = torch.Generator().manual_seed(11)
    n_rays, S = 12, 256
    rays = torch.zeros(n_rays, 13)
    rays[:, 0:3] = torch.rand(n_rays, 3, generator=gen) * 0.3 - 0.15
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=1)
    rays[:, 11], rays[:, 12] = 0.02, 0.6
    z = torch.sort(torch.rand(n_rays, S, generator=gen) * 0.55 + 0.02, dim=1).values
    d_sigma = torch.randn(n_rays, S, generator=gen)
    scale = torch.ones(n_rays, 1)
    scale[1::2] = 2.0 ** -30
    _, _, d0 = _run(ops, spec_h, params, d_sigma, rays=rays, z=z)
    _, _, d1 = _run(ops, spec_h, params, d_sigma * scale, rays=rays, z=z)
    assert float(d0[:, 0:6].abs().min()) > 0.0
    bad = [r for r in range(n_rays) if not torch.equal(d1[r], d0[r] * float(scale[r]))]
    assert not bad, f"rays whose d_rays did not scale exactly: {bad} (max rel {max(rel(d1[r], d0[r] * float(scale[r])) for r in bad):.1e})"

