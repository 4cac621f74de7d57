"""The truth, the yardstick and the cases for render_forward, render_backward and los_loss_fused (loner_amd/csrc/lnr_render.hip,
lnr_render_ray.h) at every sample tier.

The forward and the loss are oracle.render.composite and oracle.loss.lidar_loss: both compute in the dtype of what they are given, so
float64 in is the truth and float32 in is the noise yardstick.  Gradients come from autograd with respect to sigma and the ray record;
z is a constant, as in the kernels.

The backward cancels: d_alpha = G T - suffix / tt is a difference of two terms that nearly cancel where G = dL/dw is nearly constant
along the ray (an L1 selection on a ray whose target is zero).  A ray's d_sigma is then T_end-sized while each term is G T_i-sized, and
a float32 evaluation - the oracle's own - errs by many times the ray's largest d_sigma entry.  The gradients are therefore held to the
size of the terms they are the difference of (`term_magnitudes`), from the float64 run only.

`ray_parts`, `kernel_G_*` and `manual_backward` spell out the per-sample quantities the magnitudes need and the order of operations of
the kernels; tests/test_render_host.py ties them to the oracle and to autograd, and applies the slips a kernel could make to them.

Two magnitudes go beyond a block's largest entry, each for a term that a float32 evaluation cannot avoid and that the oracle's own
float32 run need not show:
  - The transmittance T_i is a product of one factor exp(-delta r) per earlier sample of positive density (the others are exactly 1).
    Each factor carries up to 1 ulp of the exponential and half an ulp of the multiplication, and an exponential whose error leans
    one way adds them up: `growth` (ray_parts) is 1 + (3/8) k_i for k_i such factors, so that the bound's 4 ulp grow by 1.5 ulp per
    factor.  It multiplies the weights' magnitude and the terms of `term_magnitudes`; a ray that is dense at all 2048 samples (ray 12
    of every case) is thus allowed 3e-4 of its largest weight, one with 20 samples in its surface 2e-6.
  - G of render_backward contains the variance's path through depth, itself a cancelling sum: `render_G_magnitude`.
The per-ray scalars depth, opacity and variance are sums over a ray's weights and are held per ray to `forward_magnitudes`, not to
the largest entry of the case: measured on an MI355X at S = 2047, ray 3 (opacity 0.15: a thin surface of many small alphas) was off
by 26 ulp of the case's largest variance and 7 ulp of its largest opacity, where the float32 run of one CPU was off by 1.3 and 0.3 and
that of another by twice as much - 1.9 times the bound 4 x noise + 4 ulp of the largest entry with the first CPU's noise, 0.99 with
the second's - and 0.012 of 4 ulp of the ray's own magnitude.  The far column of render_backward is gD_tot (1 - opacity) and inherits
the same terms (`kernel_G_render`; 1.1 times its earlier bound at S = 2047 with the first CPU's noise).
The per-ray statistics of the fused loss (mean, sd, js, eps: ray_stats columns 3..6) are held per ray to magnitudes that come from
their conditioning (`statistics_magnitudes`), not from the largest entry of the case: js is a function of g - mean, a difference of
two 50 m-sized numbers, and moves by |d js / d mean| times whatever the mean moves by.
  - mean = sum s_i w_i / wden, wden = opacity + 1e-10: sum |s_i| w_i f_i / wden, f = the `growth` of the weights above.
  - var = sum q_i^2 w_i / wden + 1e-10, q = s - mean: the sum of its terms, sum q_i^2 w_i f_i / wden + 1e-10, plus what the mean's
    own error moves it by, |2 sum q_i w_i / wden| mag(mean) (the derivative with respect to the centre; nearly 0 about the true mean,
    not about another centre).  sd = sqrt(var) follows through d sd / d var = 1 / (2 sd).
  - js = gaussian_js(g, min_eps / 3, mean, sd): |d js / d mean| mag(mean) + |d js / d sd| mag(sd) from float64 autograd of the oracle's
    gaussian_js, plus the sum of the absolute values of the terms of its two KL expressions (log, quotient, 0.5; each halved).
  - eps = min_eps (1 + js_alpha score) under the JS selections: min_eps js_alpha mag(js).  Under the LOS selections eps is the
    configured float32 number, bit for bit.
Four terms that a float32 evaluation cannot avoid go beyond that list.  With the list alone the oracle's own float32 run errs by up to
1000 times 4 ulp of sd's magnitude (S = 64, ray 19) and 63 times js's; with them it stays below 0.32 of 4 ulp of every magnitude, and
a float32 run whose exponential leans by 2^-23 of its value at every sample below 0.63 (tests/test_render_host.py):
  - alpha_i = 1 - e_i has no relative accuracy of its own: it carries the ABSOLUTE error of e_i, up to an ulp of e_i, however small
    alpha_i is.  In a sum over the ray w_i enters with w_i f_i + e_i T_i / 2 where its density is positive (`weight_terms`), in mean and
    var alike; on a ray of 1024 samples with alpha = 0.005 each that is 100 times the weights themselves.  At the other end, where
    e_k is small, alpha_k = fl(1 - e_k) is rounded by a quarter of an ulp of 1 (or by all of e_k, if that is less), which the factor
    tt_k = 1 - alpha_k + 1e-10 inherits as an absolute error: every weight behind a sample that absorbs nearly everything carries
    min(e_k, ulp / 4) / tt_k relative, summed over such k in a_i (behind one factor tt = 5.7e-4, S = 2, ray 11: 1e-5 of the weight
    that decides that ray's sd).
  - s_i = z_i scale is rounded to float32 before mean is subtracted: q_i carries half an ulp of s_i, independently per sample, and var
    moves by sum 2 |q_i| |s_i| w_i / wden.  (The list's |2 sum q_i w_i / wden| has the absolute value outside the sum: it covers a
    common shift of every q_i, not this.)
  - where var is its 1e-10 floor (one sample holds all the weight) the square of the mean's own error shows: 4 ulp mag(mean)^2.
  - g = depth_gt scale is rounded to float32 as well, and js depends on g - mean: |d js / d mean| |g|.

The fused loss refuses S > 1024 (LNR_LOSS_MAX_SAMPLES; DESIGN.md 3.5: refused, cause unknown): its cases are LOSS_SAMPLE_COUNTS."""
import functools

import torch

from oracle import loss as OL
from oracle import render as ORD
from tests.tail_restatement import F32_EPS, Ledger, block_err, block_max     # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64


def f32(x):
    """the value a float argument of the library holds"""
    return float(torch.tensor(x, dtype=F32))


N_RAYS = 26
SHALLOW = 3                                  # the ray whose surface lies at depth 0.02
DENSE = 12                                   # the ray whose density is positive at every sample
SCALE = f32(85.76)
SELECTIONS = ("L1_JS", "L2_JS", "L1_LOS", "L2_LOS")
FIXED_EPS = f32(3.0 * 0.95 ** 3)             # the LOS selections' margin at iteration 3
DEPTH_LAMBDA = f32(0.005)
TIER_EDGES = {1: (2, 63, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512), 16: (513, 1000, 1024), 32: (1025, 2047, 2048)}
SAMPLE_COUNTS = tuple(S for edges in TIER_EDGES.values() for S in edges)
LOSS_MAX_SAMPLES = 1024                      # LNR_LOSS_MAX_SAMPLES: the fused loss refuses more
LOSS_SAMPLE_COUNTS = tuple(S for S in SAMPLE_COUNTS if S <= LOSS_MAX_SAMPLES)


def chunk_for(S):
    """samples per lane (lnr_render_ray.h: chunk_for)"""
    c, p = (S + 63) // 64, 1
    while p < c:
        p <<= 1
    return p


def loss_config(selection):
    """oracle configuration with the values the library's float32 LossConfig holds"""
    return OL.LossConfig(selection=selection, depth_lambda=DEPTH_LAMBDA, eps0=FIXED_EPS, decay_eps=False)


# ---------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def case(S, seed=0):
    """26 rays of S samples, float32: dict(sigma, noise, dens, z, rays, depth_gt).  dens = sigma + noise formed here in float32 is what
    the reference receives as its density; the kernel receives sigma and noise and forms the same sum, so relu cannot differ.

    z sorted uniform in [0.02, 0.90]; |d| in [0.9, 1.1]; far 0.95, ray 0 0.70 (far[0] is what every depth_gt is compared with);
    depth_gt in [0.15, 0.68] (opaque) apart from rays 1, 8, 15, 22 (0: no return), 4, 11, 18, 25 (0.80 > far[0]: transparent), ray 9
    (0.76: transparent) and ray 3 (0.02: its target window reaches depth 0, where a kernel's padding slots would sit; its bump is
    9 exp(..) - 3 of width 1.5 m, 4 m behind the surface: it stays partly transparent, and its js selects a margin wider than its depth).
    Three families in rotation: a bump 40 exp(-((s - c - off) / width)^2 / 2) - 3 + 0.5 randn (metres) with off = 0 and width 0.25 to
    1.5 m; the same with off = 0.6 m; plain 20 randn.  c is the ray's depth_gt, or a random depth where there is no return.
    Ray 12 sits on a floor of +6 instead of -3: every one of its samples has a positive density, as on a scan through a wall."""
    gen = torch.Generator().manual_seed(1000 * S + seed)
    n = N_RAYS
    u = lambda *shape: torch.rand(*shape, generator=gen, dtype=F64)
    z = torch.sort(0.02 + 0.88 * u(n, S), dim=1).values.float()
    rays = torch.zeros(n, 13, dtype=F64)
    rays[:, 0:3] = u(n, 3) - 0.5
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=F64), dim=1) * (0.9 + 0.2 * u(n, 1))
    rays[:, 3:6], rays[:, 6:9] = d, -d
    rays[:, 11], rays[:, 12] = 1.0 / 85.76, 0.95
    rays[0, 12] = 0.70
    depth_gt = 0.15 + 0.53 * u(n)
    centre = depth_gt.clone()
    idx = torch.arange(n)
    none, clear = idx % 7 == 1, idx % 7 == 4
    depth_gt[none], depth_gt[clear] = 0.0, 0.80
    centre[clear] = 0.80
    depth_gt[9] = centre[9] = 0.76
    depth_gt[SHALLOW] = centre[SHALLOW] = 0.02
    width = 0.25 + 1.25 * u(n)
    width[0::6] = 0.25 + 0.35 * u(n)[0::6]          # narrow bumps on the surface: the rays whose js can fall below min_js
    amplitude, base = torch.full((n,), 40.0, dtype=F64), torch.full((n,), -3.0, dtype=F64)
    width[SHALLOW], amplitude[SHALLOW] = 1.5, 9.0        # thin, and (below) 4 m behind its surface: js widens its window down to depth 0
    base[DENSE] = 6.0
    off = torch.where(idx % 3 == 1, 0.6, 0.0).double()
    off[SHALLOW] = 4.0
    s = z.double() * SCALE
    bump = amplitude[:, None] * torch.exp(-0.5 * ((s - (centre * SCALE + off)[:, None]) / width[:, None]) ** 2) + base[:, None] \
        + 0.5 * torch.randn(n, S, generator=gen, dtype=F64)
    plain = 20.0 * torch.randn(n, S, generator=gen, dtype=F64)
    sigma = torch.where((idx % 3 == 2)[:, None], plain, bump).float()
    noise = torch.randn(n, S, generator=gen, dtype=F64).float()

    def away_from_zero(x, fix):
        for _ in range(8):
            bad = x.abs() < 1e-3
            if not bool(bad.any()):
                break
            x = fix(bad)
        return x
    sigma = away_from_zero(sigma, lambda bad: torch.where(bad, torch.full_like(sigma, 2e-3), sigma))
    state = dict(noise=noise)

    def move_noise(bad):
        state["noise"] = torch.where(bad, state["noise"] + 0.5, state["noise"])
        return sigma + state["noise"]
    dens = away_from_zero(sigma + noise, move_noise)
    return dict(S=S, sigma=sigma, noise=state["noise"], dens=dens, z=z, rays=rays.float(), depth_gt=depth_gt.float())


# ---------------------------------------------------------------- forward, loss and their autograd
def forward(dens, z, rays):
    """oracle.render.composite on the ray record's direction and far columns"""
    return ORD.composite(dens, z, rays[:, 3:6], rays[:, 12:13])


def cotangents(S, seed=0):
    """float32 cotangents of (depth, weights, opacity, variance) for render_backward"""
    gen = torch.Generator().manual_seed(77 + 13 * S + seed)
    return dict(depth=torch.randn(N_RAYS, generator=gen), weights=torch.randn(N_RAYS, S, generator=gen),
                opacity=torch.randn(N_RAYS, generator=gen), variance=torch.randn(N_RAYS, generator=gen))


def render_scalar(out, cot):
    """sum of cot * output over the outputs that have a cotangent"""
    return sum((out[k] * c.to(out[k].dtype)).sum() for k, c in cot.items() if c is not None)


def render_grads(dens, z, rays, cot):
    """autograd of render_scalar -> (d_sigma [n,S], d_rays [n,13]) in the dtype of the inputs"""
    dens, rays = dens.detach().clone().requires_grad_(True), rays.detach().clone().requires_grad_(True)
    g = torch.autograd.grad(render_scalar(forward(dens, z, rays), cot), (dens, rays))
    return g[0], g[1]


def loss_run(dens, z, rays, depth_gt, selection, far0=None, eps_frozen=None, scale=SCALE):
    """oracle.loss.lidar_loss on oracle.render.composite with autograd, in the dtype of the inputs -> dict(out, loss, terms, aux,
    d_sigma, d_rays).  eps_frozen [n,1]: the margin is this tensor instead of what js selects (for finite differences)."""
    dens, rays = dens.detach().clone().requires_grad_(True), rays.detach().clone().requires_grad_(True)
    out = forward(dens, z, rays)
    loss, aux = _lidar_loss(out, z, rays, depth_gt, selection, far0, eps_frozen, scale)
    g = torch.autograd.grad(loss, (dens, rays))
    return dict(out={k: v.detach() for k, v in out.items()}, loss=loss.detach(), terms=[t.detach() for t in aux["terms"]], aux=aux,
                d_sigma=g[0], d_rays=g[1])


def _lidar_loss(out, z, rays, depth_gt, selection, far0=None, eps_frozen=None, scale=SCALE):
    cfg = loss_config(selection)
    if eps_frozen is None:
        return OL.lidar_loss(out, z, rays, depth_gt, scale, cfg, 0, far0=far0)
    # frozen margin: the LOS form of the loss takes eps as it is given; a [n,1] tensor broadcasts through target_weights
    cfg = OL.LossConfig(selection=selection.replace("JS", "LOS"), depth_lambda=DEPTH_LAMBDA, eps0=eps_frozen, decay_eps=False)
    return OL.lidar_loss(out, z, rays, depth_gt, scale, cfg, 0, far0=far0)


def eps_of(aux, n, dtype):
    """the per-ray margin as a tensor [n]"""
    e = aux["eps"]
    return e.reshape(-1).to(dtype) if torch.is_tensor(e) else torch.full((n,), float(e), dtype=dtype)


# ---------------------------------------------------------------- per-sample parts (the kernels' own quantities)
def ray_parts(dens, z, rays, gaps=None):
    """delta (scaled by |d|), e = exp(-delta relu(dens)), tt = 1 - alpha + 1e-10, T (exclusive product of tt), w, and the per-ray sums,
    in the dtype of the inputs.  gaps [n,S]: sample spacings to use instead of z's own (before the |d| scaling)."""
    dnorm = torch.linalg.vector_norm(rays[:, 3:6], dim=1)
    if gaps is None:
        gaps = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones_like(z[:, :1])], dim=1)
    delta = gaps * dnorm[:, None]
    r = torch.relu(dens)
    e = torch.exp(-delta * r)
    tt = 1.0 - (1.0 - e) + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(tt[:, :1]), tt], dim=1), dim=1)[:, :-1]
    w = (1.0 - e) * T
    opacity = w.sum(1)
    far = rays[:, 12]
    depth = (w * z).sum(1) + (1.0 - opacity) * far
    variance = (w * (depth[:, None] - z) ** 2).sum(1)
    pos = dens > 0
    before = torch.cumsum(pos.to(w.dtype), dim=1) - pos.to(w.dtype)          # factors other than 1 in T_i
    return dict(delta=delta, e=e, tt=tt, T=T, w=w, r=r, pos=pos, dnorm=dnorm, opacity=opacity, depth=depth, variance=variance,
                z=z, far=far, dirs=rays[:, 3:6], growth=1.0 + 0.375 * before)


def suffix_exclusive(x):
    """sum over k > i along the ray"""
    return torch.flip(torch.cumsum(torch.flip(x, [1]), 1), [1]) - x


def kernel_G_render(p, cot, slip=None):
    """dL/dw of render_scalar as render_backward_kernel forms it -> (G [n,S], gD_tot [n], |.| pieces for the far magnitude)"""
    n = p["w"].shape[0]
    zero = torch.zeros(n, dtype=p["w"].dtype)
    get = lambda k: cot[k].to(p["w"].dtype) if cot.get(k) is not None else zero
    gD, gO, gV = get("depth"), get("opacity"), get("variance")
    q = p["depth"][:, None] - p["z"]
    through = gV * 2.0 * (p["w"] * q).sum(1)
    gD_tot = gD if slip == "c" else gD + through
    G = gO[:, None] + gD_tot[:, None] * (p["z"] - p["far"][:, None]) + gV[:, None] * q * q
    if cot.get("weights") is not None:
        G = G + cot["weights"].to(G.dtype)
    # the far column gD_tot (1 - opacity): the terms of gD_tot with the weights at the size of what they are formed from and the depth
    # inside q at its own magnitude, times |1 - opacity|; plus gD_tot times what the opacity itself can be off by (forward_magnitudes)
    fm = forward_magnitudes(p)
    gD_mag = gD.abs() + gV.abs() * 2.0 * ((weight_terms(p) * q.abs()).sum(1) + p["opacity"].abs() * fm["depth"])
    far_mag = gD_mag * (1.0 - p["opacity"]).abs() + gD_tot.abs() * fm["opacity"]
    return G, gD_tot, far_mag


def render_G_magnitude(p, cot):
    """The size of the terms G of render_backward is the sum of.  The variance's path through depth, gV 2 sum_k w_k (D - z_k), is
    itself a sum that cancels (it equals -gV 2 (1 - opacity) (D - far): exactly 0 on an opaque ray), so |G| alone understates what a
    float32 evaluation of G can resolve: that path enters with sum_k w_k |D - z_k|."""
    n = p["w"].shape[0]
    zero = torch.zeros(n, dtype=p["w"].dtype)
    get = lambda k: cot[k].to(p["w"].dtype).abs() if cot.get(k) is not None else zero
    gD, gO, gV = get("depth"), get("opacity"), get("variance")
    q = p["depth"][:, None] - p["z"]
    gD_mag = gD + gV * 2.0 * (p["w"] * q.abs()).sum(1)
    mag = gO[:, None] + gD_mag[:, None] * (p["z"] - p["far"][:, None]).abs() + gV[:, None] * q * q
    return mag + cot["weights"].to(mag.dtype).abs() if cot.get("weights") is not None else mag


def loss_pieces(p, depth_gt, selection, far0, counts, eps, pad_slots=0):
    """The fused loss as los_loss_ray forms it from the parts, in the dtype of the parts -> dict(G, gD, target, per-ray terms).
    eps [n]: the margins (taken from the oracle's run).  counts = (n_all rays, n_opaque).  pad_slots: slip (e) - that many extra
    samples at depth 0 are counted into the target's normaliser."""
    dtype = p["w"].dtype
    cfg = loss_config(selection)
    n, S = p["w"].shape
    opaque = (depth_gt > 0) & ~(depth_gt > far0)
    s, g = p["z"] * SCALE, (depth_gt * SCALE)[:, None]
    if pad_slots:
        padded = torch.cat([s, torch.zeros(n, pad_slots, dtype=dtype)], dim=1)
        target = OL.target_weights(padded, g, eps[:, None])[:, :S]
    else:
        target = OL.target_weights(s, g, eps[:, None])
    target = torch.where(opaque[:, None], target, torch.zeros_like(target))
    n_all, n_op = float(counts[0]) * S, float(counts[1])
    diff = p["w"] - target
    depth_m = p["depth"] * SCALE
    op = opaque.to(dtype)
    gO = op * torch.sign(p["opacity"] - 1.0) / n_op
    gD = op * cfg.depth_lambda * 2.0 * (depth_m - g[:, 0]) * SCALE / n_op
    if selection.startswith("L1"):
        gw, los = torch.sign(diff), diff.abs().sum(1)
    else:
        gw, los = 2.0 * diff, (diff * diff).sum(1)
    G = cfg.los_lambda * gw / n_all + gO[:, None] + gD[:, None] * (p["z"] - p["far"][:, None])
    terms = dict(depth=op * cfg.depth_lambda * (depth_m - g[:, 0]) ** 2 / n_op, los=cfg.los_lambda * los / n_all,
                 opacity=op * (p["opacity"] - 1.0).abs() / n_op)
    terms["total"] = terms["depth"] + terms["los"] + terms["opacity"]
    far_mag = gD.abs() * (1.0 - p["opacity"]).abs()
    return dict(G=G, gD=gD, target=target, diff=diff, terms=terms, opaque=opaque, far_mag=far_mag)


def manual_backward(p, G, gD_tot, slip=None):
    """render_ray_backward in the dtype of the parts -> (d_sigma [n,S], d_rays [n,13]).  slip "a": the suffix sum includes its own
    sample; slip "d": the far column lacks the factor (1 - opacity)."""
    gw = G * p["w"]
    suffix = suffix_exclusive(gw) + (gw if slip == "a" else 0.0)
    d_alpha = G * p["T"] - suffix / p["tt"]
    d_x = d_alpha * p["e"]
    d_sigma = torch.where(p["pos"], d_x * p["delta"], torch.zeros_like(d_x))
    d_norm = (d_x * p["r"] * (p["delta"] / p["dnorm"][:, None])).sum(1)
    d_rays = torch.zeros(G.shape[0], 13, dtype=G.dtype)
    d_rays[:, 3:6] = d_norm[:, None] * p["dirs"] / p["dnorm"][:, None]
    d_rays[:, 12] = gD_tot if slip == "d" else gD_tot * (1.0 - p["opacity"])
    return d_sigma, d_rays


def lane_gap_slip(z, C):
    """slip (b): the gap after a lane's last sample (positions C L + C - 1) is taken from two samples on"""
    S = z.shape[1]
    gaps = torch.cat([z[:, 1:] - z[:, :-1], 1e10 * torch.ones_like(z[:, :1])], dim=1)
    pos = torch.arange(C - 1, S - 2, C)
    gaps[:, pos] = z[:, pos + 2] - z[:, pos]
    return gaps


def term_magnitudes(p, G):
    """The size of what a gradient entry is the difference of, from a float64 run (G: dL/dw, or the size of the terms it is the sum
    of where those cancel: render_G_magnitude):
    M_i = (|G_i| T_i f_i + sum_{k>i} |G_k| w_k f_k / tt_i) e_i delta_i where dens_i > 0 (the entry is exactly 0 elsewhere) -> [n,S],
    f = the product's growth;
    D = sum_i M_i relu(dens_i) / |d| for the direction columns -> [n]"""
    f = p["growth"]                                                            # the error of the product T_i: module docstring
    M = (G.abs() * p["T"] * f + suffix_exclusive(G.abs() * p["w"] * f) / p["tt"]) * p["e"] * p["delta"]
    M = torch.where(p["pos"], M, torch.zeros_like(M))
    D = (M * p["r"]).sum(1) / p["dnorm"]
    return M, D


def total_G(dens, z, rays, scalar_of):
    """G = dL/dw as a total derivative, float64: opacity, depth and variance re-expressed through a detached leaf w.
    scalar_of(rendered dict) -> the scalar to differentiate."""
    w = forward(dens, z, rays)["weights"].detach().clone().requires_grad_(True)
    opacity = w.sum(1)
    depth = (w * z).sum(1) + (1.0 - opacity) * rays[:, 12]
    variance = (w * (depth[:, None] - z) ** 2).sum(1)
    return torch.autograd.grad(scalar_of(dict(weights=w, opacity=opacity, depth=depth, variance=variance)), w)[0]


# ---------------------------------------------------------------- per-ray statistics of the fused loss (ray_stats columns 3..6)
STAT_NAMES = ("mean", "sd", "js", "eps")
STAT_SLIPS = ("f", "g", "h")


def ray_statistics(p, depth_gt, selection, slip=None):
    """mean, sd, js, eps [n,4] as los_loss_ray forms them from the parts, in the dtype of the parts.  Slips a kernel could make:
    "f": the variance is taken about depth * scale (the rendered depth, which the kernel holds as well) instead of the mean;
    "g": the variance's sum is not divided by wden;  "h": a js below min_js is not set to 0 before it selects the margin."""
    cfg = loss_config(selection)
    dtype = p["w"].dtype
    s, g = p["z"] * SCALE, depth_gt.to(dtype) * SCALE
    wden = p["opacity"] + 1e-10
    mean = (s * p["w"]).sum(1) / wden
    centre = p["depth"] * SCALE if slip == "f" else mean
    v = ((s - centre[:, None]) ** 2 * p["w"]).sum(1)
    sd = torch.sqrt((v if slip == "g" else v / wden) + 1e-10)
    js = OL.gaussian_js(g, cfg.min_eps / 3.0, mean, sd)
    if selection.endswith("JS"):
        score = js.clone()
        if slip != "h":
            score[score < cfg.min_js] = 0
        score[score > cfg.max_js] = cfg.max_js
        eps = cfg.min_eps * (1 + cfg.js_alpha * score)
    else:
        eps = torch.full_like(js, FIXED_EPS)
    return torch.stack([mean, sd, js, eps], dim=1)


def weight_terms(p):
    """per sample the size of what w_i = (1 - e_i) T_i is formed from, for sums over a ray: w_i (f_i + a_i) + e_i T_i / 2 (module
    docstring; with the half the bound's 4 ulp allow e_i an error of 2^-22 e_i, which is 2 to 4 of its own ulps)"""
    zero = torch.zeros_like(p["w"])
    lost = torch.where(p["pos"], torch.clamp(p["e"] * 2.0 ** 21, max=1.0 / 16.0) / p["tt"], zero)      # min(e_k, ulp / 4) / tt_k over the bound's 4 ulp
    absorbed = torch.cumsum(lost, dim=1) - lost
    return p["w"] * (p["growth"] + absorbed) + torch.where(p["pos"], 0.5 * p["e"] * p["T"], zero)


def forward_magnitudes(p):
    """per ray the size of what opacity = sum w_i, depth = sum w_i z_i + (1 - opacity) far and variance = sum w_i (depth - z_i)^2 are
    formed from -> dict of [n] (float64 parts): the weights enter as `weight_terms`; the depth inherits the opacity's through far, the
    variance the depth's through d variance / d depth = 2 sum w_i q_i"""
    assert p["w"].dtype == F64
    wt = weight_terms(p)
    opacity = wt.sum(1)
    depth = (wt * p["z"].abs()).sum(1) + (1.0 - p["opacity"]).abs() * p["far"].abs() + opacity * p["far"].abs()
    q = p["depth"][:, None] - p["z"]
    variance = (wt * q * q).sum(1) + (2.0 * (p["w"] * q).sum(1)).abs() * depth
    return dict(opacity=opacity, depth=depth, variance=variance)


def statistics_magnitudes(p, depth_gt, selection):
    """per ray the size of what mean, sd, js and eps are formed from (module docstring), from float64 parts -> [n,4]"""
    assert p["w"].dtype == F64
    cfg = loss_config(selection)
    s, g = p["z"] * SCALE, depth_gt.double() * SCALE
    w, wt = p["w"], weight_terms(p)
    wden = p["opacity"] + 1e-10
    mean = (s * w).sum(1) / wden
    mean_mag = (s.abs() * wt).sum(1) / wden
    q = s - mean[:, None]
    var = (q * q * w).sum(1) / wden + 1e-10
    var_mag = (q * q * wt).sum(1) / wden + 1e-10 + (2.0 * q.abs() * s.abs() * w).sum(1) / wden \
        + (2.0 * (q * w).sum(1) / wden).abs() * mean_mag + 4.0 * F32_EPS * mean_mag ** 2
    sd = torch.sqrt(var)
    sd_mag = var_mag / (2.0 * sd)
    m, d = mean.clone().requires_grad_(True), sd.clone().requires_grad_(True)
    s1 = torch.full_like(g, cfg.min_eps / 3.0)
    d_mean, d_sd = torch.autograd.grad(OL.gaussian_js(g, s1, m, d).sum(), (m, d))
    mm, sm = 0.5 * (g + mean), 0.5 * torch.sqrt(s1 ** 2 + sd ** 2)
    kl_terms = lambda m1, a, b: torch.log(b / a).abs() + (a * a + (m1 - mm) ** 2) / (2 * (b * b)) + 0.5
    js_mag = d_mean.abs() * (mean_mag + g.abs()) + d_sd.abs() * sd_mag + 0.5 * kl_terms(g, s1, sm) + 0.5 * kl_terms(mean, sd, sm)
    eps_mag = cfg.min_eps * cfg.js_alpha * js_mag if selection.endswith("JS") else torch.zeros_like(js_mag)
    return torch.stack([mean_mag, sd_mag, js_mag, eps_mag], dim=1)


def oracle_statistics(r, n):
    """mean, sd, js, eps [n,4] of a loss_run"""
    aux = r["aux"]
    return torch.stack([aux["mean"], aux["std"], aux["js"], eps_of(aux, n, aux["js"].dtype)], dim=1)


# ---------------------------------------------------------------- decisions
def ulp32(x):
    return F32_EPS * x.abs()


def decided(z, depth_gt, far0, aux, w, target, selection):
    """per ray: no discrete decision of the fused loss lies close enough to its threshold for float32 to take it the other way"""
    cfg = loss_config(selection)
    n = z.shape[0]
    s, g = z.double() * SCALE, depth_gt.double() * SCALE
    eps = eps_of(aux, n, F64)
    ok = torch.ones(n, dtype=torch.bool)
    for edge in (g - eps, g + eps):
        near = (s - edge[:, None]).abs() <= 1e-5 * torch.maximum(s.abs(), edge.abs()[:, None])
        ok &= ~near.any(1)
    if selection.endswith("JS"):                                               # under the LOS selections js selects nothing
        js = aux["js"].double()
        for thr in (cfg.min_js, cfg.max_js):
            ok &= (js - thr).abs() > 1e-4 * thr
    if selection.startswith("L1"):
        diff = (w - target).abs()
        close = (diff > 0) & (diff < 64.0 * ulp32(torch.maximum(w.abs(), target.abs())))
        ok &= ~close.any(1)
    d = depth_gt.double()
    ok &= ((d - float(far0)).abs() > 4.0 * F32_EPS * abs(float(far0))) & ((d == 0) | (d.abs() > 4.0 * 2.0 ** -149))
    return ok


# ---------------------------------------------------------------- references per case (shared, never modified)
def _dd(x):
    return x.double()


@functools.lru_cache(maxsize=None)
def forward_reference(S):
    """the forward on the noisy density in float32 and float64, and the weights' magnitude per ray"""
    c = case(S)
    f64 = forward(_dd(c["dens"]), _dd(c["z"]), _dd(c["rays"]))
    p = ray_parts(_dd(c["dens"]), _dd(c["z"]), _dd(c["rays"]))
    return dict(f32=forward(c["dens"], c["z"], c["rays"]), f64=f64, weights_mag=(f64["weights"] * p["growth"]).max(1).values,
                mag=forward_magnitudes(p))


COTANGENT_SETS = ("all", "depth", "variance")


def cot_set(S, which):
    cot = cotangents(S)
    return cot if which == "all" else {k: (v if k == which else None) for k, v in cot.items()}


@functools.lru_cache(maxsize=None)
def backward_reference(S, which):
    """render_backward on the noisy density: float32 and float64 autograd and the float64 term magnitudes"""
    c = case(S)
    cot = cot_set(S, which)
    dens, z, rays = c["dens"], c["z"], c["rays"]
    g32 = render_grads(dens, z, rays, cot)
    g64 = render_grads(_dd(dens), _dd(z), _dd(rays), cot)
    p = ray_parts(_dd(dens), _dd(z), _dd(rays))
    G = total_G(_dd(dens), _dd(z), _dd(rays), lambda out: render_scalar(out, cot))
    M, D = term_magnitudes(p, torch.maximum(G.abs(), render_G_magnitude(p, cot)))
    _, _, far_mag = kernel_G_render(p, cot)
    return dict(cot=cot, g32=g32, g64=g64, M=M, D=D, far_mag=far_mag, G=G, parts=p)


@functools.lru_cache(maxsize=None)
def loss_reference(S, selection):
    """the fused loss on the noisy case"""
    c = case(S)
    n_rays = N_RAYS
    dens, z, rays, dgt = (c[k] for k in ("dens", "z", "rays", "depth_gt"))
    r32 = loss_run(dens, z, rays, dgt, selection)
    r64 = loss_run(_dd(dens), _dd(z), _dd(rays), _dd(dgt), selection)
    far0 = rays[0, 12]
    opaque = r64["aux"]["opaque"]
    counts = (n_rays, int(opaque.sum()))
    p = ray_parts(_dd(dens), _dd(z), _dd(rays))
    G = total_G(_dd(dens), _dd(z), _dd(rays), lambda out: _lidar_loss(out, _dd(z), _dd(rays), _dd(dgt), selection)[0])
    M, D = term_magnitudes(p, G)
    eps64 = eps_of(r64["aux"], n_rays, F64)
    pieces = loss_pieces(p, _dd(dgt), selection, float(far0), counts, eps64)
    ok = decided(z, dgt, far0, r64["aux"], r64["out"]["weights"], r64["aux"]["target"], selection)
    stats = dict(f32=oracle_statistics(r32, n_rays), f64=ray_statistics(p, _dd(dgt), selection), mag=statistics_magnitudes(p, _dd(dgt), selection))
    return dict(r32=r32, r64=r64, counts=counts, opaque=opaque, far0=far0, M=M, D=D, far_mag=pieces["far_mag"], G=G, parts=p,
                pieces=pieces, decided=ok, eps64=eps64, stats=stats)


def loss_terms(S, selection, keep, dtype):
    """(total, depth, los, opacity, sum of eps) of the oracle over the rays `keep` (bool [N_RAYS]), in `dtype`, with far[0] and the
    normalisers of the whole batch: the oracle's means over the kept rays are scaled back to the batch's counts"""
    c = case(S)
    ref = loss_reference(S, selection)
    dens, z, rays, dgt = (c[k][keep].to(dtype) for k in ("dens", "z", "rays", "depth_gt"))
    _, aux = _lidar_loss(forward(dens, z, rays), z, rays, dgt, selection, far0=ref["far0"].to(dtype))
    n_sub, n_op_sub = int(keep.sum()), int(aux["opaque"].sum())
    depth, los, opacity = (t.detach() for t in aux["terms"])
    depth, opacity = depth * (n_op_sub / ref["counts"][1]), opacity * (n_op_sub / ref["counts"][1])
    los = los * (n_sub / ref["counts"][0])
    return torch.stack([depth + los + opacity, depth, los, opacity, eps_of(aux, n_sub, dtype).sum()])


def loss_term_magnitudes(ref, keep):
    """per term the largest single ray's contribution (float64) times the number of rays"""
    t = ref["pieces"]["terms"]
    n = int(keep.sum())
    per_ray = [t["total"], t["depth"], t["los"], t["opacity"], ref["eps64"]]
    return [float(x[keep].abs().max()) * n for x in per_ray]


# ---------------------------------------------------------------- blocks and their bound
def row_blocks(x32, x64, mag=None):
    """per row: (error of the float32 run, the block's magnitude).  The float32 error is not taken below the median relative float32
    error of these rows times the row's magnitude: one row that happened to round well sets no unreachable bar."""
    x32, x64 = x32.detach().double().reshape(x64.shape[0], -1), x64.detach().double().reshape(x64.shape[0], -1)
    ref_max = x64.abs().max(1).values
    mag = ref_max if mag is None else torch.maximum(ref_max, mag.double().reshape(-1))
    err = (x32 - x64).abs().max(1).values
    live = mag > 0
    rel = torch.where(live, err / torch.where(live, mag, torch.ones_like(mag)), torch.zeros_like(mag))
    floor = rel[live].median() if bool(live.any()) else torch.tensor(0.0, dtype=F64)
    return torch.maximum(err, floor * mag), mag


def limit(noise, mag):
    """the project's bound: 4 x float32 noise + 4 ulp of the block's magnitude"""
    return 4.0 * noise + 4.0 * F32_EPS * mag


def check_rows(led, name, x, x32, x64, mag=None, where=""):
    """every row of x (the kernel's, or a slipped restatement's) as a block against the float64 rows"""
    noise, mag = row_blocks(x32, x64, mag)
    x, x64 = x.detach().cpu().double().reshape(x64.shape[0], -1), x64.detach().double().reshape(x64.shape[0], -1)
    err = (x - x64).abs().max(1).values
    ok = True
    for i in range(x64.shape[0]):
        ok &= led.figures(name, float(err[i]), float(noise[i]), float(mag[i]), f"{where} ray {i}")
    return ok


def check_statistics(led, x, ref, keep, where="", prefix=""):
    """mean, sd, js, eps (x [kept rays, 4]: ray_stats columns 3..6, or a slipped restatement's) per ray on the rays `keep`"""
    st = ref["stats"]
    ok = True
    for k, name in enumerate(STAT_NAMES):
        ok &= check_rows(led, prefix + name, x[:, k], st["f32"][keep, k], st["f64"][keep, k], st["mag"][keep, k], where)
    return ok


def check_case(led, name, x, x32, x64, mag=None, where=""):
    """one block for the whole case: a per-ray scalar, or the far column"""
    ref_max = block_max(x64)
    return led.figures(name, block_err(x, x64), block_err(x32, x64), ref_max if mag is None else max(ref_max, float(mag)), where)
