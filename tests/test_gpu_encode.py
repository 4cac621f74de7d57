"""encode_forward, encode_backward and table_grad_reduce against the float64 continuation of tests/encode_restatement.py, PER LEVEL,
per table entry, per point and per ray - needs an MI355X.

The MLP is a selector (encode_restatement.selector_params): sigma = sum_j c_j feature_j with c a one-hot vector (forward: sigma IS
feature j) or c_j = 2^-(j mod 8) (backward: every d_feature plane is an exact power-of-two multiple of d_sigma), so what is compared
is the arithmetic of the encode kernels alone.  The default network runs it on both MLP kernels of its shape class (precision
"fp32" and "fp32_chain", ReLU pair relu(s) - relu(-s)), the others with activation None.

Bounds - none is taken from the kernel:
  block (one level's table gradient; d_pts and d_rays column triples): 4 x the error of the restatement's float32 run + 4 ulp of the
      block's largest entry (tail_restatement.bound), for a table level plus the record budget at the level's largest A_e;
  table entry e:  A_e x 2^-17 + n_e x 2^-42 + 4 ulp of |ref_e|, A_e the sum of the absolute contributions and n_e their number:
      2^-17 for the 26-bit record values (2^-18), the 28-bit fx and the fp32 products and run sums; 2^-42 per contribution for the
      fixed-point sum (2^-43 rounding, two products per x-pair).  hash_f1 (fp32 records): 2^-21 instead of 2^-17;
  point:  32 x 2^-24 x (sum of the absolute terms of the point's input gradient): 32 roundings between a table value and d_pts;
  ray:  A_r x 2^-17 + n_r x 2^-42 + 4 ulp, A_r the sum of the absolute terms over the ray's samples (times z for the direction
      columns) and n_r = levels x ceil(S / 64): ray_accumulate_dx adds one __float2ll_rn(0.5 v 2^42) per wave and level, 2^-43 each.
"""
import functools
import re

import pytest
import torch

from tests import encode_restatement as ER
from tests.test_gpu_kernels import NETS

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
ALL_DENSE = dict(otype="HashGrid", n_levels=2, n_features_per_level=2, log2_hashmap_size=19, base_resolution=4, per_level_scale=2.0)
# (encoding, neurons of the selector's hidden layer, the precisions it runs in)
CASES = {"default": (NETS["default"][0], 64, ("fp32", "fp32_chain")), "hash_f1": (NETS["hash_f1"][0], 16, ("fp32",)),
         "hash_f4_2hidden": (NETS["hash_f4_2hidden"][0], 64, ("fp32",)), "hash_f8": (NETS["hash_f8"][0], 32, ("fp32",)),
         "all_dense": (ALL_DENSE, 32, ("fp32",))}
NET_PREC = [(n, p) for n, c in CASES.items() for p in c[2]]
TABLE_GAIN = 3000.0


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


@functools.lru_cache(maxsize=None)
def _grid_table(name):
    from loner_amd import hip
    grid = ER.make_grid(CASES[name][0])
    spec = hip.make_net_spec(CASES[name][0], dict(activation="None", n_neurons=16, n_hidden_layers=1))
    for l, lv in enumerate(grid.levels):
        # the library's own float32 scale: exp2f(l log2f(growth)) may differ by an ulp between C libraries, and the scale defines the cell
        assert (lv.res, lv.size, lv.offset, int(lv.hashed)) == (spec.level_res[l], spec.level_size[l], spec.level_offset[l], spec.level_hashed[l])
        assert abs(lv.scale - spec.level_scale[l]) <= 2e-7 * lv.scale
        lv.scale = float(spec.level_scale[l])
    gen = torch.Generator().manual_seed(17)
    return grid, (torch.rand(grid.n_entries * grid.n_features, generator=gen) * 2 - 1) * 1e-4 * TABLE_GAIN


def _network(name, prec, coeff):
    """-> (library spec, parameter vector on the device) of the selector sum_j coeff[j] feature_j over the table of _grid_table"""
    from loner_amd import hip
    enc, neurons, _ = CASES[name]
    relu = name == "default"
    net = dict(activation="ReLU" if relu else "None", n_neurons=neurons, n_hidden_layers=1, precision=prec)
    spec = hip.make_net_spec(enc, net)
    grid, table = _grid_table(name)
    enc_dim = len(grid.levels) * grid.n_features
    in_dim = (enc_dim + 15) // 16 * 16
    mlp = ER.selector_params([(neurons, in_dim), (16, neurons)], int(spec.n_mlp_params), coeff, relu)
    assert int(spec.n_params) == mlp.numel() + table.numel()
    return spec, dv(torch.cat([mlp, table]))


def _record_rel(name):
    return ER.RECORD_REL_F32 if name == "hash_f1" else ER.RECORD_REL


@functools.lru_cache(maxsize=None)
def _points(name):
    """1000 random points and the crafted ones"""
    grid, _ = _grid_table(name)
    gen = torch.Generator().manual_seed(23)
    crafted, _ = ER.crafted_points(grid, 0)
    return torch.cat([torch.rand(1000, 3, generator=gen) * 1.98 - 0.99, crafted])


@functools.lru_cache(maxsize=None)
def _crafted(name):
    return ER.crafted_points(_grid_table(name)[0], 0)[0]


def _d_feat(grid, d_sigma):
    coeff = torch.tensor(ER.all_level_coefficients(len(grid.levels) * grid.n_features), dtype=F64)
    return d_sigma.double().reshape(-1, 1) * coeff[None, :]


@functools.lru_cache(maxsize=4)
def _reference(name, which):
    """(points [n,3], d_sigma, live mask or None, float32 run, float64 run, per-point magnitude) of a named batch, computed once"""
    grid, table = _grid_table(name)
    live = None
    if which == "crafted":
        p = _crafted(name)
        d_sigma = ER.sweep_d_sigma(p.shape[0])
    elif which.startswith("rays"):
        S = int(which[4:])
        rays, z, n_live = ER.bunched_rays(S)
        p = ER.world_points(rays, z).reshape(-1, 3)
        d_sigma = torch.randn(8 * S, generator=torch.Generator().manual_seed(S))
        d_sigma[1::5] = 0.0
        live = torch.arange(8 * S) < n_live * S
    else:
        rays, z, d_sigma = _skewed_batch()
        p = ER.world_points(rays, z).reshape(-1, 3)
        d_sigma = d_sigma.reshape(-1)
    d_feat = _d_feat(grid, d_sigma)
    r32 = ER.encode(grid, table, p, F32, d_feat.float(), live)
    r64 = ER.encode(grid, table, p, F64, d_feat, live)
    for key in ("A", "cnt", "feat"):
        r32[key] = None
    mag = None if which == "skewed" else ER.input_magnitude(grid, table, p, d_feat, live)
    return p, d_sigma, live, r32, r64, mag


def _check_table(led, case, name, grad, r32, r64, scale=1.0, base=None):
    """ER.check_table on the grid of `name` with its record precision"""
    ER.check_table(led, case, _grid_table(name)[0], grad, r32, r64, _record_rel(name), scale, base)


_check_points = ER.check_points


# ------------------------------------------------------------------------------------------- a. forward, per feature
@pytest.mark.parametrize("name,prec", NET_PREC)
def test_forward_every_feature_against_float64(ops, name, prec):
    grid, table = _grid_table(name)
    p = _points(name)
    f32 = torch.cat(ER.encode(grid, table, p, F32)["feat"], dim=1)
    f64 = torch.cat(ER.encode(grid, table, p, F64)["feat"], dim=1)
    led = ER.EncodeLedger()
    F = grid.n_features
    for j in range(f64.shape[1]):
        coeff = [0.0] * f64.shape[1]
        coeff[j] = 1.0
        spec, params = _network(name, prec, coeff)
        sigma = ops.density_forward(spec, params, pts=dv(p))
        led.block(f"forward {name} {prec}: feature of level {j // F:2d}", sigma.cpu(), f32[:, j], f64[:, j], f"feature {j}")
    _finish(led)


# ------------------------------------------------------------------------------------------- b. crafted points, points form
@pytest.mark.parametrize("name,prec", NET_PREC)
def test_backward_on_crafted_points_per_level_entry_and_point(ops, name, prec):
    """x cells with 0 .. all trailing one bits on every x-pair level (12 and more: the corners straddle owner slices and travel as two
    single-corner records), x fractions of exactly 0 and as close to 1 as a float32 coordinate gets, points on the six faces and up to
    35 % outside them (hashed levels included: cells wrap)"""
    grid, _ = _grid_table(name)
    p, d_sigma, _, r32, r64, mag = _reference(name, "crafted")
    spec, params = _network(name, prec, ER.all_level_coefficients(len(grid.levels) * grid.n_features))
    grad = torch.zeros(int(spec.n_params), device=DEV)
    d_pts = ops.density_backward(spec, params, dv(d_sigma), grad, pts=dv(p), want_d_pts=True)
    led = ER.EncodeLedger()
    _check_table(led, f"crafted {name} {prec}", name, grad, r32, r64)
    _check_points(led, f"crafted {name} {prec}", d_pts, r32, r64, mag)
    _finish(led)


# ------------------------------------------------------------------------------------------- c. / f. run-length combining, rays form
def _rays_case(ops, prec, S, mode):
    name = "default"
    grid, _ = _grid_table(name)
    rays, z, n_live = ER.bunched_rays(S)
    p, d_sigma, live, r32, r64, mag = _reference(name, f"rays{S}")
    spec, params = _network(name, prec, ER.all_level_coefficients(len(grid.levels) * grid.n_features))
    n_dev = torch.tensor([n_live], dtype=torch.int32, device=DEV)
    R, Z, D = dv(rays), dv(z), dv(d_sigma.reshape(8, S))
    led = ER.EncodeLedger()
    case = f"rays S={S} {prec} {mode}"
    gen = torch.Generator().manual_seed(3)
    if mode == "accumulate":
        base = torch.randn(int(spec.n_params), generator=gen)
        grad = dv(base)
        ops.density_backward(spec, params, D, grad, rays=R, z=Z, n_rays_dev=n_dev)
        _check_table(led, case, name, grad, r32, r64, base=base)
    elif mode == "overwrite":
        grad = torch.full((int(spec.n_params),), 7.0, device=DEV)
        ops.density_backward(spec, params, D, grad, rays=R, z=Z, n_rays_dev=n_dev, overwrite_grad=True)
        _check_table(led, case, name, grad, r32, r64)
    else:
        grad = torch.zeros(int(spec.n_params), device=DEV)
        d_pts = ops.density_backward(spec, params, D, grad, rays=R, z=Z, n_rays_dev=n_dev, want_d_pts=True)
        _check_table(led, case, name, grad, r32, r64)
        _check_points(led, case, d_pts, r32, r64, mag, live=live)
        # the per-ray reduction: in-wave (S a multiple of 64) or through planes (S = 100)
        base = torch.randn(8, 13, generator=gen)
        d_rays = dv(base)
        grad2 = torch.zeros_like(grad)
        assert ops.density_backward(spec, params, D, grad2, rays=R, z=Z, n_rays_dev=n_dev, d_rays=d_rays) is None
        assert torch.equal(grad2[int(spec.n_mlp_params):], grad[int(spec.n_mlp_params):])
        out = d_rays.cpu()
        assert torch.equal(out[n_live:], base[n_live:]) and torch.equal(out[:, 6:], base[:, 6:])         # dead rows and other columns untouched
        s32 = ER.ray_sums(sum(r32["dpts"]).reshape(8, S, 3), z)
        s64 = ER.ray_sums(sum(r64["dpts"]).reshape(8, S, 3), z)
        got = (out[:, :6].double() - base[:, :6].double())[:n_live]
        a_o = mag.reshape(8, S).sum(dim=1)
        a_d = (mag.reshape(8, S) * z.double()).sum(dim=1)
        n_r = len(grid.levels) * ((S + 63) // 64)
        for cols, a, what in ((slice(0, 3), a_o, "origin"), (slice(3, 6), a_d, "direction")):
            # (d_rays = base + sum: the sum is rounded once more onto |base| <= 5, half an ulp of the result)
            slack = ER.F32_EPS * (base[:n_live, cols].double().abs() + s64[:n_live, cols].abs())
            led.budget_block(f"{case}: d_rays {what} columns", got[:, cols], s32[:n_live, cols], s64[:n_live, cols], float(slack.max()))
            limit = (a[:n_live] * ER.RECORD_REL + n_r * ER.FIX_STEP)[:, None] + 4.0 * ER.F32_EPS * s64[:n_live, cols].abs() + slack
            led.elements(f"{case}: d_rays {what} per ray", got[:, cols], s64[:n_live, cols], limit)
    _finish(led)


@pytest.mark.parametrize("prec", ["fp32", "fp32_chain"])
@pytest.mark.parametrize("S", [64, 128, 100])
def test_run_length_combining_along_rays(ops, prec, S):
    """8 rays x S samples with bunches of samples 1e-6 apart: runs of one cell inside a 16-lane row, across rows, waves, a partition
    batch and up to the ray's end (tests/test_encode_host.py checks that they are there); 7 live rays"""
    _rays_case(ops, prec, S, "plain")


@pytest.mark.parametrize("mode", ["accumulate", "overwrite"])
def test_gradient_accumulates_into_or_overwrites_the_buffer(ops, mode):
    _rays_case(ops, "fp32", 128, mode)


# ------------------------------------------------------------------------------------------- d. overflow and the split reduce
def _skewed_batch():
    """the batch of test_record_partition_under_worst_skew_equals_global_accumulation (test_gpu_kernels.py) - every sample in three clusters of a few cells, stragglers
    elsewhere - with 512 rays instead of 256: the library gives the dense-indexed levels several reduce workgroups per owner only
    from 32 partition chunks (65 536 samples) on"""
    gen = torch.Generator().manual_seed(12)
    N, S = 512, 128
    rays = torch.zeros(N, 13)
    rays[:, 0:3] = torch.tensor([0.05, -0.02, 0.01]); rays[:, 3:6] = torch.tensor([0.6, 0.0, 0.8]); rays[:, 6:9] = -rays[:, 3:6]
    rays[:, 11] = 0.01; rays[:, 12] = 0.8
    z = torch.full((N, S), 0.2) + torch.rand(N, S, generator=gen) * 1e-6
    z[:, 40:80] += 0.1; z[:, 80:] += 0.25
    z[::17, ::9] = torch.rand(len(range(0, N, 17)), len(range(0, S, 9)), generator=gen) * 0.7 + 0.02
    z = torch.sort(z, dim=1).values
    return rays, z, torch.randn(N, S, generator=gen)


def test_region_overflow_and_split_reduce_against_float64(ops, capfd):
    name, prec = "default", "fp32"
    grid, _ = _grid_table(name)
    rays, z, d_sigma = _skewed_batch()
    p, _, _, r32, r64, mag = _reference(name, "skewed")
    spec, params = _network(name, prec, ER.all_level_coefficients(len(grid.levels) * grid.n_features))
    grad = torch.zeros(int(spec.n_params), device=DEV)
    capfd.readouterr()
    ops.density_backward(spec, params, dv(d_sigma), grad, rays=dv(rays), z=dv(z), report_regions=True)
    torch.cuda.synchronize()
    report = capfd.readouterr().err
    rows = re.findall(r"level +(\d+): (\d+)-B records, capacity (\d+), mean [\d.]+, max (\d+), overflowed \d+ of \d+, "
                      r"overflow accumulators (used|unused), (\d+) reduce workgroups per owner", report)
    assert len(rows) == len(grid.levels), report
    hashed_overflow = [int(l) for l, _, cap, mx, used, _ in rows if grid.levels[int(l)].hashed and used == "used" and int(mx) >= int(cap)]
    split = [int(l) for l, *_, parts in rows if int(parts) > 1]
    print("regions that filled up and overflowed on hashed levels:", hashed_overflow, " levels reduced by several workgroups per owner:", split)
    assert hashed_overflow, report
    assert split and all(not grid.levels[l].hashed for l in split), report
    led = ER.EncodeLedger()
    _check_table(led, "skewed 512 x 128", name, grad, r32, r64)
    _finish(led)


# ------------------------------------------------------------------------------------------- e. magnitudes
@pytest.mark.parametrize("prec", ["fp32", "fp32_chain"])
def test_magnitude_sweep_of_d_sigma(ops, prec):
    """d_sigma 2^k on the crafted points, k = -40 .. 14: the reference scales exactly.  From |value| >= 256 on the fixed-point
    conversion takes its generic branch (k = 8, 14; k = 8 has x-pairs with one value on either side, tests/test_encode_host.py); at the
    small end the sum's 2^-42 resolution takes over from the records' 2^-17: a contribution below 2^-25 is resolved to less than that."""
    name = "default"
    grid, _ = _grid_table(name)
    p, d_sigma, _, r32, r64, mag = _reference(name, "crafted")
    spec, params = _network(name, prec, ER.all_level_coefficients(len(grid.levels) * grid.n_features))
    led = ER.EncodeLedger()
    for k in ER.SWEEP_EXPONENTS:
        scale = 2.0 ** k
        grad = torch.zeros(int(spec.n_params), device=DEV)
        d_pts = ops.density_backward(spec, params, dv(d_sigma * scale), grad, pts=dv(p), want_d_pts=True)
        _check_table(led, f"2^{k:+d} {prec}", name, grad, r32, r64, scale=scale)
        _check_points(led, f"2^{k:+d} {prec}", d_pts, r32, r64, mag, scale=scale)
        # which term of the entry bound is the larger one, over the touched entries of the x-pair levels
        floor = sum(int(((r64["cnt"][l] * ER.FIX_STEP > r64["A"][l] * scale * ER.RECORD_REL) & (r64["cnt"][l] > 0)).sum())
                    for l in range(len(grid.levels)))
        touched = sum(int((r64["cnt"][l] > 0).sum()) for l in range(len(grid.levels)))
        print(f"FIGURES d_sigma 2^{k:+d}: n_e 2^-42 exceeds A_e 2^-17 on {floor} of {touched} touched entries")
    _finish(led)
