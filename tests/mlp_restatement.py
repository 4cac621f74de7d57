"""Dtype-generic restatement of the density MLP of the default shape class - 32 encoded features -> H <= 64 ReLU neurons -> sigma, no
biases, row 0 of the 16-row output matrix - with its analytic backward, and the dyadic-lattice inputs on which that network has ONE
correct bit pattern: the reference of tests/test_gpu_mlp_default.py.

Plain torch, no import of oracle/ (`launch` alone asks the library for a launch shape, on the host): tests/test_mlp_host.py ties the float32 run to oracle/network.py, the
float64 run to its autograd, and a lattice sub-case to a rational evaluation of the published algorithm (tests/known_answer.py).

Every function computes in the dtype it is given.  float64 is the truth.  The float32 run adds its terms one after the other in index
order (no blocked or pairwise sums: those are more accurate than a kernel has to be) and is the noise yardstick of
tail_restatement.bound.  Beside every output the backward returns A, the sum of the absolute values of the terms the output is the sum
of: rounding errors of any evaluation order scale with it.

THE LATTICE.  With per_level_scale = 2 and base_resolution = 2 the level scales are the integers 2^(l+1) - 1.  A world coordinate that
is a multiple of 1/d (d a power of two) has the unit coordinate k / 2d, the position k scale / 2d + 1/2 and a fraction that is a multiple
of 1/2d; the eight corner weights are multiples of 1/(2d)^3, and with table values n / t the features are multiples of 1/((2d)^3 t).
With weights m / w every product and every partial sum of the network, in ANY order, is an integer number of a stage's lsb (the
product of its operands' lsbs); while the sum of the absolute terms stays below 2^24 lsb each of them is a float32 number, so float32
arithmetic of any association, tile shape or operand split returns the float64 result bit for bit (`exact_budget`)."""
import math

import numpy as np
import torch

from tests import encode_restatement as ER

F32, F64 = torch.float32, torch.float64
IN_DIM = 32

# 16 levels x 2 features with integer scales 1, 3, 7 ... 65535; levels 0-3 dense, 4-15 hashed into 4096 entries
LATTICE_ENC = dict(otype="HashGrid", n_levels=16, n_features_per_level=2, log2_hashmap_size=12, base_resolution=2, per_level_scale=2.0)
# world coordinates k / denominator; table values n / table_den, weights m / weight_den with |n|, |m| up to the alphabets' ends
FINE = dict(name="fine", denominator=4, table_alphabet=tuple(range(-8, 9)), table_den=16, weight_alphabet=tuple(range(-4, 5)), weight_den=8)
COARSE = dict(name="coarse", denominator=2, table_alphabet=(-1, 0, 1), table_den=1, weight_alphabet=tuple(range(-2, 3)), weight_den=4)
D_SIGMA_ALPHABET = (1.0, -1.0, 0.5, -0.5)
D_SIGMA_LSB = 0.5


# ---------------------------------------------------------------- the network
def unpack(params, H):
    """MLP part of a flat parameter vector -> (W1 [H,32], W_out [16,H])"""
    return params[:H * IN_DIM].reshape(H, IN_DIM), params[H * IN_DIM:H * IN_DIM + 16 * H].reshape(16, H)


def pack(W1, wo):
    """(W1 [H,32], wo [H]) -> the MLP part of a parameter vector: W1, then the 16-row output matrix with wo as row 0"""
    out = torch.zeros(16, W1.shape[0], dtype=W1.dtype)
    out[0] = wo
    return torch.cat([W1.reshape(-1), out.reshape(-1)])


def _sequential(dtype, sequential):
    return dtype == F32 if sequential is None else sequential


def preactivations(feat, W1, sequential=None):
    """Z [n,H] = feat [n,32] W1^T; sequential (default: in float32): the 32 products are added one after the other"""
    if not _sequential(feat.dtype, sequential):
        return feat @ W1.T
    Z = torch.zeros(feat.shape[0], W1.shape[0], dtype=feat.dtype)
    for k in range(feat.shape[1]):
        Z = Z + feat[:, k, None] * W1[None, :, k]
    return Z


def mlp(feat, W1, wo, sequential=None):
    """-> (sigma [n], Z [n,H]) in the dtype of the arguments"""
    Z = preactivations(feat, W1, sequential)
    hid = torch.relu(Z)
    if not _sequential(feat.dtype, sequential):
        return hid @ wo, Z
    sigma = torch.zeros(feat.shape[0], dtype=feat.dtype)
    for j in range(W1.shape[0]):
        sigma = sigma + hid[:, j] * wo[j]
    return sigma, Z


def _sample_sums(d_sigma, dZ, hid, feat, sequential):
    """dW1 [H,32] = sum_s dZ_s (x) feat_s and dWo [H] = sum_s d_sigma_s hid_s; sequential: sample by sample, in order"""
    if not sequential:
        return dZ.T @ feat, d_sigma @ hid
    dW1 = torch.zeros(dZ.shape[1], feat.shape[1], dtype=feat.dtype)
    dWo = torch.zeros(dZ.shape[1], dtype=feat.dtype)
    for s in torch.nonzero(d_sigma)[:, 0].tolist():              # (a sample with d_sigma == 0 adds zeros)
        dW1.addr_(dZ[s], feat[s])
        dWo.add_(hid[s] * d_sigma[s])
    return dW1, dWo


def backward(feat, W1, wo, d_sigma, sequential=None, round_dz=None):
    """The analytic backward of sum_s d_sigma_s sigma_s, in the dtype of the arguments -> dict:
    sigma [n], Z [n,H], dZ [n,H] (= d_sigma wo where Z > 0, else 0), dW1 [H,32], dWo [H], d_feature [n,32], and the sums of absolute
    terms A_sigma [n], A_dW1 [H,32], A_dWo [H], A_d_feature [n,32] (float64 whatever the dtype).  round_dz: applied to dZ before its
    two products (the fp16 storage model)."""
    seq = _sequential(feat.dtype, sequential)
    sigma, Z = mlp(feat, W1, wo, seq)
    hid = torch.relu(Z)
    dZ = torch.where(Z > 0, d_sigma[:, None] * wo[None, :], torch.zeros_like(Z))
    if round_dz is not None:
        dZ = round_dz(dZ)
    dW1, dWo = _sample_sums(d_sigma, dZ, hid, feat, seq)
    if seq:
        d_feat = torch.zeros_like(feat)
        for j in range(W1.shape[0]):
            d_feat = d_feat + dZ[:, j, None] * W1[None, j, :]
    else:
        d_feat = dZ @ W1
    # (sigma and dWo are sums of products of SUMS: their terms are those of the expanded sum over the live neurons' 32 products)
    z64, f64 = dZ.double().abs(), feat.double().abs()
    a_hid = (f64 @ W1.double().abs().T) * (Z > 0)
    return dict(sigma=sigma, Z=Z, dZ=dZ, dW1=dW1, dWo=dWo, d_feature=d_feat, A_sigma=a_hid @ wo.double().abs(), A_dW1=z64.T @ f64,
                A_dWo=d_sigma.double().abs() @ a_hid, A_d_feature=z64 @ W1.double().abs())


def round_f16(x):
    return x.to(torch.float16).to(x.dtype)


def backward_f16_storage(feat, W1, wo, d_sigma):
    """`backward` with the storage roundings of the fp16 mode (oracle/network.py, precision "fp16": features and both weight matrices
    to fp16, products accumulated unrounded, the hidden activation feeds the output row unrounded) and the kernels' fp16 dZ operand"""
    return backward(round_f16(feat), round_f16(W1), round_f16(wo), d_sigma, round_dz=round_f16)


# ---------------------------------------------------------------- lattice builders
def lattice_grid():
    return ER.make_grid(LATTICE_ENC)


def _choice(alphabet, n, gen):
    return torch.tensor(alphabet, dtype=F64)[torch.randint(0, len(alphabet), (n,), generator=gen)]


def lattice_table(alphabet, denominator, seed):
    """float32 [entries x 2] of the lattice encoding: values a / denominator, a drawn from `alphabet`"""
    grid = lattice_grid()
    gen = torch.Generator().manual_seed(seed)
    return (_choice(alphabet, grid.n_entries * grid.n_features, gen) / denominator).float()


def lattice_weights(H, alphabet, denominator, seed):
    """-> (W1 [H,32], wo [H]) float32, values a / denominator; no output weight is zero (a neuron would drop out of sigma and dW1)"""
    gen = torch.Generator().manual_seed(seed + 1000 * H)
    W1 = (_choice(alphabet, H * IN_DIM, gen) / denominator).reshape(H, IN_DIM).float()
    wo = (_choice([a for a in alphabet if a != 0], H, gen) / denominator).float()
    return W1, wo


def lattice_axis(denominator):
    return torch.arange(-denominator, denominator + 1, dtype=F64) / denominator


def distinct_lattice_points(denominator):
    a = lattice_axis(denominator)
    return torch.cartesian_prod(a, a, a).float()


def lattice_points(n, denominator, seed):
    """float32 [n,3]: one random permutation of all (2 denominator + 1)^3 lattice points after the other, so that every distinct point
    occurs (n >= their number) and no two neighbours are equal"""
    distinct = distinct_lattice_points(denominator)
    m = distinct.shape[0]
    assert n >= m
    gen = torch.Generator().manual_seed(seed)
    order, last = [], -1
    while sum(o.numel() for o in order) < n:
        perm = torch.randperm(m, generator=gen)
        if int(perm[0]) == last:
            perm = perm.roll(1)
        order.append(perm)
        last = int(perm[-1])
    return distinct[torch.cat(order)[:n]].contiguous()


def lattice_d_sigma(n, seed, dead=(0, 0), live_share=0.125, block=16):
    """float32 [n]: values of D_SIGMA_ALPHABET on a random `live_share` of the samples, exactly 0 elsewhere and on all of [dead[0],
    dead[1]); every aligned block of `block` samples with a sample outside the dead stretch holds a live one (forced where chance left
    none), and so does every block of a multiple of `block` samples"""
    gen = torch.Generator().manual_seed(seed)
    d = _choice(D_SIGMA_ALPHABET, n, gen).float()
    d = d * (torch.rand(n, generator=gen) < live_share)
    forced = _choice(D_SIGMA_ALPHABET, n, gen).float()
    alive = torch.ones(n, dtype=torch.bool)
    alive[dead[0]:dead[1]] = False
    d = d * alive
    for b in range((n + block - 1) // block):
        lo, hi = b * block, min(n, (b + 1) * block)
        if bool(alive[lo:hi].any()) and not bool((d[lo:hi] != 0).any()):
            s = lo + int(torch.nonzero(alive[lo:hi])[0, 0])
            d[s] = forced[s]
    return d


def lattice_rays(n_rays, S, denominator, seed):
    """-> (rays [n_rays,13], z [n_rays,S]) float32: origins on the lattice, direction a signed unit axis, z sorted multiples of the
    lattice step that keep o + d z inside the cube - the product and the sum are exact, the samples lie on the lattice"""
    gen = torch.Generator().manual_seed(seed)
    axis_values = lattice_axis(denominator)
    o = axis_values[torch.randint(0, axis_values.numel(), (n_rays, 3), generator=gen)]
    axis = torch.randint(0, 3, (n_rays,), generator=gen)
    sign = torch.randint(0, 2, (n_rays,), generator=gen).double() * 2 - 1
    d = torch.zeros(n_rays, 3, dtype=F64)
    d[torch.arange(n_rays), axis] = sign
    room = torch.round((1.0 - sign * o[torch.arange(n_rays), axis]) * denominator)          # lattice steps up to the face ahead
    steps = torch.floor(torch.rand(n_rays, S, generator=gen, dtype=F64) * (room[:, None] + 1)).clamp(max=room[:, None])
    z = torch.sort(steps, dim=1).values / denominator
    rays = torch.zeros(n_rays, 13, dtype=F64)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6:9], rays[:, 11], rays[:, 12] = o, d, -d, 0.0, 2.0
    return rays.float(), z.float()


def lattice_features(grid, table, pts, dtype):
    """[n,32] in `dtype`: ER.encode on the distinct points, gathered"""
    distinct, inverse = torch.unique(pts, dim=0, return_inverse=True)
    return torch.cat(ER.encode(grid, table, distinct, dtype)["feat"], dim=1)[inverse]


# ---------------------------------------------------------------- exactness
def significant_bits(x):
    """largest number of significand bits between the leading and the last set bit over the non-zero float32 entries of x"""
    v = x.detach().reshape(-1).numpy().astype(np.float32)
    v = v[v != 0]
    if v.size == 0:
        return 0
    mant = (v.view(np.uint32) & np.uint32(0x7FFFFF)) | np.uint32(0x800000)          # (the lattices hold no subnormal numbers)
    low = mant & (~mant + np.uint32(1))
    return int(24 - np.log2(low.astype(np.float64)).min())


def _lsb(x):
    """the largest power of two that divides every entry of x"""
    v = x.detach().double().reshape(-1)
    v = v[v != 0]
    e = 0
    while bool((torch.round(v * 2.0 ** e) != v * 2.0 ** e).any()):
        e += 1
        assert e < 60
    while bool((torch.round(v * 2.0 ** (e - 1)) == v * 2.0 ** (e - 1)).all()) and e > -60:
        e -= 1
    return 2.0 ** -e


def exact_budget(feat, W1, wo, d_sigma=None):
    """Per stage the largest sum of absolute terms in units of the stage's lsb (the product of its operands' lsbs; the operands' own lsbs
    are measured): dict(preactivation, sigma[, dW1, dWo, d_feature]).  Below 2^24 every partial sum of the stage, in any order, is an
    integer number of lsbs that float32 holds exactly."""
    feat, W1, wo = feat.double(), W1.double(), wo.double()
    l_f, l_w1, l_wo = _lsb(feat), _lsb(W1), _lsb(wo)
    Z = feat @ W1.T
    hid = torch.relu(Z)
    l_z = l_f * l_w1
    out = dict(preactivation=float((feat.abs() @ W1.abs().T).max()) / l_z, sigma=float((hid @ wo.abs()).max()) / (l_z * l_wo))
    if d_sigma is not None:
        ds = d_sigma.double()
        l_dz = _lsb(ds) * l_wo
        dZ = torch.where(Z > 0, ds[:, None] * wo[None, :], torch.zeros_like(Z)).abs()
        out.update(dW1=float((dZ.T @ feat.abs()).max()) / (l_dz * l_f), dWo=float((ds.abs() @ hid).max()) / (_lsb(ds) * l_z),
                   d_feature=float((dZ @ W1.abs()).max()) / (l_dz * l_w1))
    return out


def log2_figures(budget):
    return "  ".join(f"{k} 2^{math.log2(v):.1f}" if v > 0 else f"{k} 0" for k, v in budget.items())


# ---------------------------------------------------------------- the cases of tests/test_gpu_mlp_default.py (preconditions: test_mlp_host.py)
ROUTES = {"bf3": "fp32", "fast32": "fp32_chain", "f16_fast": "fp16"}          # route -> the precision that selects it
WIDTHS = (16, 32, 64)
FORWARD_LATTICE = {"bf3": FINE, "fast32": FINE, "f16_fast": COARSE}
LATTICES = {"fine": FINE, "coarse": COARSE}
TABLE_SEED, POINT_SEED, WEIGHT_SEED, D_SIGMA_SEED, RAY_SEED = 101, 102, 103, 104, 105
RAY_SAMPLES = (96, 93)          # 96 = 3 x 32: a live count times 96 always fills its last 32-sample step; 93 leaves it ragged


def net_config(route, H):
    return dict(activation="ReLU", n_neurons=H, n_hidden_layers=1, precision=ROUTES[route])


def launch(route, H, backward, enc=None):
    """-> dict(n, grid, tile, R): the launch shape the library reports for the route at a large batch (its workgroup cap), R = grid x 4
    waves x tile = the samples of one round (one step of every wave), and the test size n = 2 R + 5 tile + 17: two full rounds, six
    waves (seven with 16-sample tiles) with a third step, the last of them on a tile that is partly filled and whose last pair holds one sample.  (The only function here that asks
    the library anything; no GPU.)"""
    from tests.support import density_route
    enc = LATTICE_ENC if enc is None else enc
    big = density_route(enc, net_config(route, H), 1 << 20, backward, shape=True)
    assert big["route"] == route, big
    R = big["grid"] * 4 * big["tile"]
    n = 2 * R + 5 * big["tile"] + 17
    assert density_route(enc, net_config(route, H), n, backward, shape=True) == big
    return dict(n=n, grid=big["grid"], tile=big["tile"], R=R)


def coordinates(sample, shape):
    """where a sample runs: (round = the wave's step, wave of the launch, workgroup, wave in it, column pair of the tile)"""
    tile_index, waves = sample // shape["tile"], shape["grid"] * 4
    wave = tile_index % waves
    return dict(step=tile_index // waves, wave=wave, workgroup=wave // 4, wave_in_workgroup=wave % 4, pair=(sample % shape["tile"]) // 2)


def waves_with_three_steps(shape):
    tiles = (shape["n"] + shape["tile"] - 1) // shape["tile"]
    return max(0, tiles - 2 * shape["grid"] * 4)


def dead_stretch(shape):
    """[lo, hi): starts inside the third tile and is 3 tiles + 6 samples longer than a round, so every wave meets it, both ends cut a
    tile and a pair, the first waves run live - dead - live and waves 3 and 4 dead - dead - live"""
    lo = 2 * shape["tile"] + 5
    return lo, lo + shape["R"] + 3 * shape["tile"] + 6


def pair_kinds(d_sigma):
    """number of pairs (2c, 2c + 1) with (both, only the even, only the odd) sample live"""
    live = d_sigma != 0
    n = live.numel() // 2 * 2
    even, odd = live[0:n:2], live[1:n:2]
    return int((even & odd).sum()), int((even & ~odd).sum()), int((~even & odd).sum())


def dead_tiles(d_sigma, tile):
    """bool per tile: no live sample"""
    n = d_sigma.numel()
    pad = torch.zeros((n + tile - 1) // tile * tile)
    pad[:n] = d_sigma
    return (pad.reshape(-1, tile) == 0).all(dim=1)


def _shares(Z):
    return float((Z > 0).double().mean()), float((Z < 0).double().mean()), float((Z == 0).double().mean())


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def lattice_inputs(lattice, n, H):
    """-> dict(grid, table, pts, W1, wo, params [n_params] float32, feat64 [n,32]) of an exact case, built once"""
    def make():
        lat = LATTICES[lattice]
        grid = lattice_grid()
        table = _cached(("table", lattice), lambda: lattice_table(lat["table_alphabet"], lat["table_den"], TABLE_SEED))
        pts = _cached(("pts", lattice, n), lambda: lattice_points(n, lat["denominator"], POINT_SEED))
        feat64 = _cached(("feat", lattice, n), lambda: lattice_features(grid, table, pts, F64))
        W1, wo = lattice_weights(H, lat["weight_alphabet"], lat["weight_den"], WEIGHT_SEED)
        return dict(grid=grid, table=table, pts=pts, W1=W1, wo=wo, params=torch.cat([pack(W1, wo), table]), feat64=feat64)
    return _cached(("inputs", lattice, n, H), make)


def forward_case(lattice, n, H):
    """lattice_inputs + sigma64 [n] of the float64 run and z_share = the share of positive, negative and zero pre-activations"""
    def make():
        c = dict(lattice_inputs(lattice, n, H))
        c["sigma64"], Z = mlp(c["feat64"], c["W1"].double(), c["wo"].double())
        c["z_share"] = _shares(Z)
        return c
    return _cached(("forward", lattice, n, H), make)


def backward_case(n, tile, R, H):
    """coarse lattice_inputs + d_sigma [n] float32, dead = (lo, hi), r64 = the float64 `backward` (without Z and dZ) and z_share"""
    def make():
        c = dict(lattice_inputs("coarse", n, H))
        c["dead"] = dead_stretch(dict(tile=tile, R=R))
        c["d_sigma"] = _cached(("d_sigma", n, c["dead"]), lambda: lattice_d_sigma(n, D_SIGMA_SEED, c["dead"]))
        c["r64"] = backward(c["feat64"], c["W1"].double(), c["wo"].double(), c["d_sigma"].double())
        c["z_share"] = _shares(c["r64"].pop("Z"))
        del c["r64"]["dZ"]
        return c
    return _cached(("backward", n, tile, R, H), make)


def rays_case(n, S):
    """-> dict(rays [n_rays,13], z [n_rays,S], live, M, pts [n_rays S, 3]): coarse-lattice rays, three more than the live ones; the live ones hold
    at most n samples, an odd number of them where S is odd, and leave the last 32-sample step ragged where S is no multiple of 32"""
    def make():
        live = n // S
        while (S % 2 == 1 and live % 2 == 0) or (S % 32 != 0 and (live * S) % 32 == 0):
            live -= 1
        n_rays = live + 3
        rays, z = lattice_rays(n_rays, S, COARSE["denominator"], RAY_SEED)
        pts = ER.world_points(rays, z).reshape(-1, 3)
        return dict(rays=rays, z=z, live=live, M=live * S, pts=pts, n_rays=n_rays)
    return _cached(("rays", n, S), make)
